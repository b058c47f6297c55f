// facade.h -- what lifecycle.cpp and routes.cpp, the two halves of the MedicalSeg:: facade, share.  Private to host/.
#pragma once
#include <algorithm>
#include <fstream>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/medseg/initialize.h"
#include "../../include/medseg/process.h"
#include "artefacts.h"

namespace MedicalSeg {

// ---- state (lifecycle.cpp)
extern std::mutex g_log_mutex;     // the reference's global log stream is written from any thread unguarded
extern std::mutex g_batch_mutex;   // the batch routes toggle group-wide state (postprocess flag): one batch call at a time
extern mi_unet_config g_cfg;       // per-rank configuration of the group (tile size, topology, max_batch, algorithm)
// contour capacities per plane of a segment call: postprocess keeps components >= 6 % of the tile, so <= 16 of them
constexpr int kCapPoints = 1 << 15, kCapContours = 64;

int env_int(const char *name, int fallback);
bool host_preprocess_requested();      // MEDSEG_HOST_PREPROCESS=1
bool device_contours_requested();      // extract_contours runs on the device behind postprocess_mask unless MEDSEG_HOST_CONTOURS=1
bool device_postprocess_requested();   // postprocess_mask runs on the device right behind the argmax unless MEDSEG_HOST_POSTPROCESS=1

// ---- the facade's settings: one owner.  Each setter (process.h) changes one field; all of them outlive the engine except the targets,
// which initialize_engine resets (the classes belong to the network being loaded).  The window is stored in Preprocess::, where the
// host routes read it, and apply() takes it from there.
struct Settings {
    std::vector<mi_unet_target> targets{ { 2, 0.06f } };
    std::vector<mi_unet_morph> morph{ { MI_UNET_MORPH_RECT, 1, 0 } };
    mi_unet_measure measure{ 0, 0 };
    std::string truth_dir;                                 // empty = off
    Volume volume;                                         // off; no handle holds it (process_image_batch reads it)
    VolumeClean volume_clean;                              // off; acts only with volume.on (process_image_batch reads it)
    VolumeMesh volume_mesh;                                // off; acts only with volume.on (process_image_batch reads it)
    VolumeInterp volume_interp;                            // off; acts only with volume.on (process_image_batch reads it)
    VolumeMeasure volume_measure;                          // off; acts only with volume.on (process_image_batch reads it)
    VolumeSpatial volume_spatial;                          // off; acts only with volume.on (process_image_batch reads it)
    VolumeSplit volume_split;                              // off; acts only with volume.on (process_image_batch reads it)
    VolumeSkeleton volume_skeleton;                        // off; acts only with volume.on (process_image_batch reads it)
    VolumeBranches volume_branches;                        // off; acts only with volume.on and volume_skeleton.on (process_image_batch reads it)
    VolumeTexture volume_texture;                          // off; acts only with volume.on (process_image_batch reads it)
    VolumeZones volume_zones;                              // off; acts only with volume.on (process_image_batch reads it)
    VolumeNbhood volume_nbhood;                            // off; acts only with volume.on (process_image_batch reads it)
    VolumeMatch volume_match;                              // off; acts only with volume.on and a truth_dir (process_image_batch reads it)
    // Hands a handle every setting it can hold -- window, measure, morphology, targets -- and returns the first refusal.  This is the one
    // way a group, a lane or a thread's context gets its settings.  Only the _multi entry points read a handle's targets and morphology
    // (include/mi_unet.h), so pushing the default lists in front of any other call is harmless.  A refusal of the DEFAULT target list
    // is not reported: a network with two classes has no class 2, and its handles keep the list they were created with.
    int apply(mi_unet_t *h) const;
    int apply(mi_unet_group_t *g) const;
};
Settings current_settings();
// get_thread_local_context(), and the settings that context has just taken
mi_unet_t *thread_context(Settings *applied);
inline bool is_default(const std::vector<mi_unet_morph> &m)
{
    return m.size() == 1 && m[0].shape == MI_UNET_MORPH_RECT && m[0].open_r == 1 && m[0].close_r == 0;
}

// plane k of a buffer of tile-sized planes, as a picture
inline medseg::Image8 tile_image(const std::vector<uint8_t> &planes, size_t k)
{
    const size_t hw = (size_t)g_cfg.height * g_cfg.width;
    medseg::Image8 m(g_cfg.height, g_cfg.width, 1);
    std::copy(planes.begin() + k * hw, planes.begin() + (k + 1) * hw, m.data.begin());
    return m;
}

// The device lanes of directory mode: the engine group and, when `second` is asked for, a clone of it with the settings in force
// (created on first use; a warning in the log when it cannot be had).  Returns their number; throws without an engine.
int device_lanes(mi_unet_group_t *lanes[2], bool second);

// routes.cpp keeps page-locked RAW buffers across calls; cleanup_resources() releases them
void release_pinned_buffers();

}  // namespace MedicalSeg
