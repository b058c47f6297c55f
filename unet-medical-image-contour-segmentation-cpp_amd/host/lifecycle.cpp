// lifecycle.cpp -- MedicalSeg::initialize_engine / cleanup_resources, the facade's state, settings, log and per-thread contexts on top
// of the C-ABI (include/mi_unet.h); the facade's units: routes.cpp.
// Reference: src/initialize.cpp:26-91, src/process.cpp:123-262, src/cleanup.cpp:10-64.
// Same log file name, banner lines, message prefixes and bool/void error conventions.  What replaces what:
//   g_runtime / g_engine (one deserialised TensorRT engine, src/initialize.cpp:20-21)
//        -> one mi_unet group: an engine handle per visible device, weights packed once and sent device-to-device
//   thread_local TensorRTContext (exec context + buffers + stream + graph per calling thread, src/process.cpp:15, :45-120)
//        -> a thread_local clone of the first device's handle (mi_unet_clone: shares the weight blob, owns buffers, stream
//           and graphs), created lazily on a thread's first single-image call, so concurrent callers do not serialise
//   the sequential file loop of directory mode (src/main.cpp:148-164)
//        -> process_image_batch: chunks of max_batch x devices images, sharded over the group
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <filesystem>
#include <iostream>
#include <stdexcept>

#include "../../include/medseg/cleanup.h"
#include "../../include/medseg/preprocess.h"
#include "facade.h"

namespace fs = std::filesystem;
using medseg::Image8;

namespace MedicalSeg {

std::mutex g_log_mutex, g_batch_mutex;
mi_unet_config g_cfg{};

namespace {
std::mutex g_state_mutex;          // guards the group, the second lane, the configuration, the generation and the settings
mi_unet_group_t *g_group = nullptr;
mi_unet_group_t *g_lane2 = nullptr;  // a clone of g_group, created by the first directory-mode call with more than one chunk
int g_thread_batch = 1;            // micro-batch capacity of a per-thread context
unsigned long g_generation = 0;    // bumped by every (re)initialisation and cleanup: older thread contexts are stale
Settings g_settings;
std::ofstream g_log_file;
std::string g_log_path;

// The calling thread's context.  Destroyed by cleanup_resources() on that thread (as the reference does, src/cleanup.cpp:16)
// or when the thread ends; a context of an older engine generation is replaced on its next use.
struct ThreadContext {
    mi_unet_t *h = nullptr;
    unsigned long generation = 0;
    void release() { if (h) { mi_unet_destroy(h); h = nullptr; } }
    ~ThreadContext() { release(); }
};
thread_local ThreadContext t_context;

int env_algo()
{
    const char *v = std::getenv("MEDSEG_CONV_ALGO");
    if (!v) return MI_UNET_CONV_AUTO;
    const std::string s(v);
    return s == "direct" ? MI_UNET_CONV_DIRECT : s == "winograd" ? MI_UNET_CONV_WINOGRAD : s == "bf16" ? MI_UNET_CONV_BF16
         : s == "fp16" ? MI_UNET_CONV_FP16 : MI_UNET_CONV_AUTO;
}

// topology of a MIUNETW1 file (miunet/spec.py): magic[8], u32 version, in_ch, base, levels, classes
// version 1, or version 2 with its u32 up_mode after the 36-byte header (miunet/spec.py); the engine validates the mode
bool read_weight_header(const std::string &path, mi_unet_config &cfg, uint32_t &up_mode)
{
    std::ifstream f(path, std::ios::binary);
    unsigned char hdr[40];
    if (!f.read(reinterpret_cast<char *>(hdr), 28) || std::memcmp(hdr, "MIUNETW1", 8) != 0) return false;
    uint32_t v[5];
    std::memcpy(v, hdr + 8, sizeof v);
    up_mode = 0;
    if (v[0] == 2) {
        if (!f.read(reinterpret_cast<char *>(hdr + 28), 12)) return false;
        std::memcpy(&up_mode, hdr + 36, 4);
    } else if (v[0] != 1) {
        return false;
    }
    cfg.in_ch = (int)v[1]; cfg.base = (int)v[2]; cfg.levels = (int)v[3]; cfg.classes = (int)v[4];
    return true;
}
}  // namespace

int env_int(const char *name, int fallback)
{
    const char *v = std::getenv(name);
    if (!v || !*v) return fallback;
    char *end = nullptr;
    const long x = std::strtol(v, &end, 10);
    return (end && *end == '\0') ? (int)x : fallback;
}

static bool env_is_1(const char *name)
{
    const char *e = std::getenv(name);
    return e && e[0] == '1';
}
bool host_preprocess_requested() { return env_is_1("MEDSEG_HOST_PREPROCESS"); }
bool device_contours_requested() { return !env_is_1("MEDSEG_HOST_CONTOURS"); }
bool device_postprocess_requested() { return !env_is_1("MEDSEG_HOST_POSTPROCESS"); }

int Settings::apply(mi_unet_t *h) const
{
    const mi_unet_window window = Preprocess::get_window();
    if (int rc = mi_unet_set_window(h, &window)) return rc;
    if (int rc = mi_unet_set_measure(h, &measure)) return rc;
    if (int rc = mi_unet_set_morph(h, morph.data(), (int)morph.size())) return rc;
    const int rc = mi_unet_set_targets(h, targets.data(), (int)targets.size());
    return is_default(targets) ? MI_UNET_OK : rc;
}

int Settings::apply(mi_unet_group_t *g) const      // every rank or none, setting by setting
{
    const mi_unet_window window = Preprocess::get_window();
    if (int rc = mi_unet_group_set_window(g, &window)) return rc;
    if (int rc = mi_unet_group_set_measure(g, &measure)) return rc;
    if (int rc = mi_unet_group_set_morph(g, morph.data(), (int)morph.size())) return rc;
    const int rc = mi_unet_group_set_targets(g, targets.data(), (int)targets.size());
    return is_default(targets) ? MI_UNET_OK : rc;
}

// Engine configuration: the topology comes from the weight file's header, everything the reference hard-codes or leaves to
// TensorRT comes from the environment --
//   MEDSEG_TILE_SIZE (or MEDSEG_TILE_W / MEDSEG_TILE_H)  network tile, default 512 (src/process.cpp:70, src/preprocess.cpp:81)
//   MEDSEG_MAX_BATCH     images per device micro-batch in directory mode, default 16
//   MEDSEG_THREAD_BATCH  capacity of a per-thread context (single-image calls), default 1
//   MEDSEG_CONV_ALGO     auto | direct | winograd | bf16 | fp16 (the arithmetic of BASELINE configs 3 and 5)
//   MEDSEG_DEVICES       number of devices in the group: default 1 (the reference's implicit device 0); N > 1 or 0 (= every
//                        visible device) is opt-in -- the multi-device transports have not met a second GPU yet
bool initialize_engine(const std::string &trt_cache_path, const std::string &log_dir)
{
    std::lock_guard<std::mutex> state_lock(g_state_mutex);
    try {
        fs::create_directories(log_dir);
        g_log_path = log_dir + "/segmentation_log.txt";
        if (g_log_file.is_open()) g_log_file.close();
        g_log_file.open(g_log_path, std::ios::out | std::ios::trunc);
        if (!g_log_file.is_open()) {
            std::cerr << "Failed to create log file: " << g_log_path << std::endl;
            return false;
        }
        g_log_file << "=== Initializing Medical Image Segmentation Engine ===" << std::endl;
        g_log_file << "MI355X UNet weight file: " << trt_cache_path << std::endl;
        if (!fs::exists(trt_cache_path)) {
            g_log_file << "Error: engine weight file not found - " << trt_cache_path << std::endl;
            return false;
        }
        if (g_lane2) { mi_unet_group_destroy(g_lane2); g_lane2 = nullptr; }
        if (g_group) { mi_unet_group_destroy(g_group); g_group = nullptr; }
        ++g_generation;
        g_settings.targets = Settings().targets;   // the classes belong to the network that is about to load
        mi_unet_default_config(&g_cfg);            // 512x512x1, 3 classes (src/process.cpp:70, :162)
        uint32_t up_mode = 0;
        if (!read_weight_header(trt_cache_path, g_cfg, up_mode)) {
            g_log_file << "Error: not a MIUNETW1 weight file - " << trt_cache_path << std::endl;
            std::cerr << "Initialization error: not a MIUNETW1 weight file" << std::endl;
            return false;
        }
        const int tile = env_int("MEDSEG_TILE_SIZE", 512);
        g_cfg.width = env_int("MEDSEG_TILE_W", tile);
        g_cfg.height = env_int("MEDSEG_TILE_H", tile);
        g_cfg.max_batch = std::max(1, env_int("MEDSEG_MAX_BATCH", 16));
        g_cfg.conv_algo = env_algo();
        g_thread_batch = std::max(1, env_int("MEDSEG_THREAD_BATCH", 1));
        const int n_devices = env_int("MEDSEG_DEVICES", 1);
        g_log_file << "Device group requested: " << (n_devices <= 0 ? std::string("every visible device") : std::to_string(n_devices))
                   << " (MEDSEG_DEVICES)" << std::endl;
        auto bring_up = [&](int devices) {
            return mi_unet_group_create(&g_cfg, nullptr, devices, &g_group) == MI_UNET_OK &&
                   mi_unet_group_load_weights(g_group, trt_cache_path.c_str()) == MI_UNET_OK;
        };
        bool up = bring_up(n_devices);
        if (!up && n_devices != 1 && mi_unet_device_count() > 1) {
            // a multi-device group that does not come up must not take single-device operation with it
            g_log_file << "Warning: multi-device group failed (" << mi_unet_last_error() << "); continuing on device "
                       << g_cfg.device << " alone" << std::endl;
            if (g_group) { mi_unet_group_destroy(g_group); g_group = nullptr; }
            up = bring_up(1);
        }
        // the other settings outlive the engine; the group may refuse them (a measured channel this network does not have)
        if (up && g_settings.apply(g_group) != MI_UNET_OK) up = false;
        if (!up) {
            g_log_file << "Error: Failed to initialize MI355X UNet engine: " << mi_unet_last_error() << std::endl;
            std::cerr << "Initialization error: " << mi_unet_last_error() << std::endl;
            if (g_group) { mi_unet_group_destroy(g_group); g_group = nullptr; }
            return false;
        }
        g_log_file << "MI355X UNet engine initialized successfully" << std::endl;
        g_log_file << "  Topology: in_ch=" << g_cfg.in_ch << " base=" << g_cfg.base << " levels=" << g_cfg.levels
                   << " classes=" << g_cfg.classes << ", tile " << g_cfg.width << "x" << g_cfg.height
                   << ", upsample=" << (up_mode == 1 ? "bilinear" : "transpose") << std::endl;
        g_log_file << "  Devices: " << mi_unet_group_size(g_group) << " (weights to ranks > 0 by "
                   << mi_unet_group_weight_transport(g_group) << "), micro-batch " << g_cfg.max_batch << " per device" << std::endl;
        g_log_file << "  " << mi_unet_numeric_guard(mi_unet_group_handle(g_group, 0), nullptr, nullptr) << std::endl;
        g_log_file << "  Input size: " << (size_t)g_cfg.height * g_cfg.width * g_cfg.in_ch << " bytes (u8)" << std::endl;
        g_log_file << "  Output size: " << (size_t)g_cfg.height * g_cfg.width << " bytes (classes=" << g_cfg.classes << ")" << std::endl;
        return true;
    } catch (const std::exception &e) {
        std::cerr << "Initialization error: " << e.what() << std::endl;
        if (g_log_file.is_open()) g_log_file << "Initialization error: " << e.what() << std::endl;
        return false;
    }
}

mi_unet_t *get_engine()
{
    std::lock_guard<std::mutex> lk(g_state_mutex);
    return g_group ? mi_unet_group_handle(g_group, 0) : nullptr;
}
mi_unet_group_t *get_engine_group() { std::lock_guard<std::mutex> lk(g_state_mutex); return g_group; }

namespace {
// The skeleton of the five setters.  Never under a running directory-mode call (the batch lock), then the state lock.  `edit` changes
// a copy of the settings and returns the reason, if any, why the rules that need no engine forbid the change.  The group, when there
// is one, takes the copy; it validates against the loaded network and may refuse, all of its ranks or none: then it takes the old
// settings back and nothing is stored.  The second lane follows the group; a thread's context takes the settings on its next use.
// `log_line` writes the stored value.  A setting that no handle holds (`handle_side` false) goes to none.
template <class Edit, class LogLine>
bool change_setting(Edit edit, LogLine log_line, bool handle_side = true)
{
    std::lock_guard<std::mutex> batch(g_batch_mutex);
    std::lock_guard<std::mutex> lk(g_state_mutex);
    Settings next = g_settings;
    std::string refused = edit(next);
    if (refused.empty() && handle_side && g_group && next.apply(g_group) != MI_UNET_OK) {
        refused = mi_unet_last_error();
        (void)g_settings.apply(g_group);
    }
    if (!refused.empty()) {
        std::cerr << "Error: " << refused << std::endl;
        return false;
    }
    if (handle_side && g_lane2) (void)next.apply(g_lane2);
    g_settings = std::move(next);
    if (g_log_file.is_open()) {
        std::lock_guard<std::mutex> ll(g_log_mutex);
        log_line(g_log_file, g_settings);
        g_log_file << std::endl;
    }
    return true;
}
}  // namespace

bool set_targets(const std::vector<Target> &targets)
{
    return change_setting(
        [&](Settings &s) {
            s.targets.clear();
            for (const Target &x : targets) s.targets.push_back({ x.cls, x.min_area_frac });
            if (targets.empty()) s.targets = Settings().targets;
            // the group validates (class range of the loaded network, repeats, fractions): without one there is nothing to set
            return std::string(g_group ? "" : "Engine not initialized");
        },
        [](std::ostream &lg, const Settings &s) {
            lg << "Targets:";
            for (const auto &x : s.targets) lg << " class " << x.cls << " (min area " << x.min_area_frac << ")";
        });
}

bool set_morphology(const std::vector<Morph> &morph)
{
    return change_setting(
        [&](Settings &s) {
            // the engine's rules (mi_unet_set_morph), which do not depend on the network: checked here, so that no engine is needed
            bool ok = morph.size() <= (size_t)MI_UNET_MAX_TARGETS;
            for (const Morph &m : morph)
                ok = ok && (m.shape == MI_UNET_MORPH_RECT || m.shape == MI_UNET_MORPH_DISC) && m.open_r >= 0 && m.open_r <= MI_UNET_MORPH_MAX_R &&
                     m.close_r >= 0 && m.close_r <= MI_UNET_MORPH_MAX_R;
            s.morph = morph.empty() ? Settings().morph : morph;
            return ok ? std::string() : "morphology: at most " + std::to_string(MI_UNET_MAX_TARGETS) + " entries of shape rect | disc with radii 0.." +
                                            std::to_string(MI_UNET_MORPH_MAX_R);
        },
        [](std::ostream &lg, const Settings &s) {
            lg << "Morphology:";
            for (const auto &m : s.morph)
                lg << " " << (m.shape == MI_UNET_MORPH_DISC ? "disc" : "rect") << " (open " << m.open_r << ", close " << m.close_r << ")";
        });
}

bool set_window(const mi_unet_window &window)
{
    return change_setting(
        // (validates and stores; the engine applies the same rules and cannot refuse)
        [&](Settings &) { return std::string(Preprocess::set_window(window) ? "" : mi_unet_last_error()); },
        [&](std::ostream &lg, const Settings &) {
            lg << "Window: mode " << window.mode << ", clip " << window.clip_lo_ppm << " / " << window.clip_hi_ppm << " ppm, fixed " << window.lo
               << " .. " << window.hi;
        });
}

bool set_measure(bool on, int channel)
{
    return change_setting(
        [&](Settings &s) {                                      // without an engine only the sign; the group knows the network's channels
            s.measure = { on ? 1 : 0, channel };
            return std::string(channel < 0 ? "measure: negative channel" : "");
        },
        [&](std::ostream &lg, const Settings &) { lg << "Measure: " << (on ? "on" : "off") << ", channel " << channel; });
}

bool set_truth_dir(const std::string &dir)
{
    return change_setting([&](Settings &s) { s.truth_dir = dir; return std::string(); },
                          [&](std::ostream &lg, const Settings &) { lg << "Truth: " << (dir.empty() ? std::string("off") : dir); },
                          /*handle_side=*/false);
}

bool set_volume(const Volume &volume)
{
    return change_setting(
        [&](Settings &s) {
            s.volume = volume;
            const bool conn = volume.connectivity == 6 || volume.connectivity == 18 || volume.connectivity == 26;
            bool spacing = true;
            for (double v : { volume.spacing_x, volume.spacing_y, volume.spacing_z }) spacing = spacing && std::isfinite(v) && v > 0.0;
            return std::string(!conn ? "volume: connectivity is 6, 18 or 26"
                               : volume.min_voxels < 0 || volume.keep_largest < 0 ? "volume: negative min_voxels or keep_largest"
                               : !spacing ? "volume: the spacing must be finite and positive" : "");
        },
        [&](std::ostream &lg, const Settings &) {
            lg << "Volume: " << (volume.on ? "on" : "off") << ", connectivity " << volume.connectivity << ", min " << volume.min_voxels << ", keep "
               << volume.keep_largest << ", spacing " << volume.spacing_x << " " << volume.spacing_y << " " << volume.spacing_z;
        },
        /*handle_side=*/false);
}

bool set_volume_clean(const VolumeClean &clean)
{
    return change_setting(
        [&](Settings &s) {
            s.volume_clean = clean;
            const bool radii = std::isfinite(clean.close_mm) && clean.close_mm >= 0.0 && std::isfinite(clean.open_mm) && clean.open_mm >= 0.0;
            return std::string(radii ? "" : "volume clean: the radii must be finite and not negative");
        },
        [&](std::ostream &lg, const Settings &) {
            lg << "Volume clean: " << (clean.on ? "on" : "off") << ", fill " << (clean.fill ? "on" : "off") << ", close " << clean.close_mm
               << " mm, open " << clean.open_mm << " mm";
        },
        /*handle_side=*/false);
}

bool set_volume_mesh(const VolumeMesh &mesh)
{
    return change_setting(
        [&](Settings &s) {
            s.volume_mesh = mesh;
            const bool placement = mesh.placement == MI_UNET_MESH_FACES || mesh.placement == MI_UNET_MESH_NETS;
            return std::string(placement ? "" : "volume mesh: the placement is MI_UNET_MESH_FACES or MI_UNET_MESH_NETS");
        },
        [&](std::ostream &lg, const Settings &) {
            lg << "Volume mesh: " << (mesh.on ? "on" : "off") << ", " << (mesh.placement == MI_UNET_MESH_NETS ? "nets" : "faces");
        },
        /*handle_side=*/false);
}

bool set_volume_interp(const VolumeInterp &interp)
{
    return change_setting(
        [&](Settings &s) {
            s.volume_interp = interp;
            const bool factor = interp.factor >= 0 && interp.factor <= MI_UNET_VINTERP_MAX_FACTOR;
            return std::string(factor ? "" : "volume interp: the factor is 0 (iso) .. MI_UNET_VINTERP_MAX_FACTOR");
        },
        [&](std::ostream &lg, const Settings &) {
            lg << "Volume interp: " << (interp.on ? "on" : "off") << ", factor " << (interp.factor ? std::to_string(interp.factor) : std::string("iso"));
        },
        /*handle_side=*/false);
}

bool set_volume_measure(const VolumeMeasure &measure)
{
    return change_setting(
        [&](Settings &s) {
            s.volume_measure = measure;
            if (measure.channel < 0) return std::string("volume measure: the channel is not negative");
            const bool cap = measure.max_ends >= 0 && measure.max_ends <= MI_UNET_VMEASURE_MAX_ENDS_LIMIT;
            return std::string(cap ? "" : "volume measure: max_ends is 0 .. MI_UNET_VMEASURE_MAX_ENDS_LIMIT");
        },
        [&](std::ostream &lg, const Settings &) {
            lg << "Volume measure: " << (measure.on ? "on" : "off") << ", channel " << measure.channel << ", ends " << measure.max_ends;
        },
        /*handle_side=*/false);
}

bool set_volume_spatial(const VolumeSpatial &spatial)
{
    return change_setting(
        [&](Settings &s) {
            s.volume_spatial = spatial;
            if (spatial.channel < 0) return std::string("volume spatial: the channel is not negative");
            if (spatial.max_voxels < 0 || spatial.max_voxels > MI_UNET_VSPATIAL_MAX_VOXELS_LIMIT)
                return std::string("volume spatial: max_voxels is 0 .. MI_UNET_VSPATIAL_MAX_VOXELS_LIMIT");
            const bool peak = std::isfinite(spatial.peak_mm) && spatial.peak_mm >= 0.0;
            return std::string(peak ? "" : "volume spatial: peak_mm is finite and not negative");
        },
        [&](std::ostream &lg, const Settings &) {
            lg << "Volume spatial: " << (spatial.on ? "on" : "off") << ", channel " << spatial.channel << ", voxels " << spatial.max_voxels << ", peak "
               << spatial.peak_mm << " mm";
        },
        /*handle_side=*/false);
}

bool set_volume_split(const VolumeSplit &split)
{
    return change_setting(
        [&](Settings &s) {
            s.volume_split = split;
            if (!(std::isfinite(split.neck_mm) && split.neck_mm >= 0.0)) return std::string("volume split: neck_mm is finite and not negative");
            return std::string(split.min_core >= 0 ? "" : "volume split: min_core is not negative");
        },
        [&](std::ostream &lg, const Settings &) {
            lg << "Volume split: " << (split.on ? "on" : "off") << ", neck " << split.neck_mm << " mm, mincore " << split.min_core;
        },
        /*handle_side=*/false);
}

bool set_volume_skeleton(const VolumeSkeleton &skeleton)
{
    return change_setting(
        [&](Settings &s) {
            s.volume_skeleton = skeleton;
            return std::string(skeleton.max_passes >= 0 ? "" : "volume skeleton: max_passes is not negative");
        },
        [&](std::ostream &lg, const Settings &) {
            lg << "Volume skeleton: " << (skeleton.on ? "on" : "off") << ", radius " << (skeleton.radius ? "on" : "off") << ", png "
               << (skeleton.png ? "on" : "off") << ", passes " << skeleton.max_passes;
        },
        /*handle_side=*/false);
}

bool set_volume_branches(const VolumeBranches &branches)
{
    return change_setting(
        [&](Settings &s) {
            s.volume_branches = branches;
            const bool ok = branches.prune_voxels >= 0 && branches.prune_voxels <= MI_UNET_VBRANCH_MAX_PRUNE && branches.prune_rounds >= 0 &&
                            branches.prune_rounds <= MI_UNET_VBRANCH_MAX_PRUNE;
            return std::string(ok ? "" : "volume branches: prune and rounds are 0 .. 1048576");
        },
        [&](std::ostream &lg, const Settings &) {
            lg << "Volume branches: " << (branches.on ? "on" : "off") << ", prune " << branches.prune_voxels << ", rounds " << branches.prune_rounds;
        },
        /*handle_side=*/false);
}

namespace {

// The five fields a texture setting (VolumeTexture, VolumeZones, VolumeNbhood) begins with: what is wrong with the first of them that is
// out of range, behind the stage's prefix ("volume texture", ...), or nothing; and their part of the log line.
template <class T>
std::string check_quantiser(const std::string &stage, const T &t)
{
    if (t.channel < 0) return stage + ": the channel is not negative";
    if (t.mode != MI_UNET_VTEX_COUNT && t.mode != MI_UNET_VTEX_WIDTH) return stage + ": the mode is MI_UNET_VTEX_COUNT or MI_UNET_VTEX_WIDTH";
    if (t.levels < 2 || t.levels > MI_UNET_VTEX_MAX_LEVELS) return stage + ": levels is 2 .. MI_UNET_VTEX_MAX_LEVELS";
    if (t.lo < 0 || t.lo > 65535) return stage + ": lo is 0 .. 65535";
    if (t.width < 1 || t.width > 65536) return stage + ": width is 1 .. 65536";
    return std::string();
}
template <class T>
std::string quantiser_text(const T &t)
{
    return std::string(t.on ? "on" : "off") + ", channel " + std::to_string(t.channel) + ", levels " + std::to_string(t.levels) + ", " +
           (t.mode == MI_UNET_VTEX_WIDTH ? "width " + std::to_string(t.width) + " lo " + std::to_string(t.lo) : std::string("count"));
}

}  // namespace

bool set_volume_texture(const VolumeTexture &texture)
{
    return change_setting(
        [&](Settings &s) {
            s.volume_texture = texture;
            return check_quantiser("volume texture", texture);
        },
        [&](std::ostream &lg, const Settings &) { lg << "Volume texture: " << quantiser_text(texture); },
        /*handle_side=*/false);
}

bool set_volume_zones(const VolumeZones &zones)
{
    return change_setting(
        [&](Settings &s) {
            s.volume_zones = zones;
            const std::string common = check_quantiser("volume zones", zones);
            if (!common.empty()) return common;
            return std::string(zones.max_run >= 2 && zones.max_run <= MI_UNET_VZONES_MAX_RUN ? "" : "volume zones: max_run is 2 .. MI_UNET_VZONES_MAX_RUN");
        },
        [&](std::ostream &lg, const Settings &) { lg << "Volume zones: " << quantiser_text(zones) << ", run " << zones.max_run; },
        /*handle_side=*/false);
}

bool set_volume_nbhood(const VolumeNbhood &nbhood)
{
    return change_setting(
        [&](Settings &s) {
            s.volume_nbhood = nbhood;
            const std::string common = check_quantiser("volume nbhood", nbhood);
            if (!common.empty()) return common;
            if (nbhood.alpha < 0 || nbhood.alpha > nbhood.levels - 1) return std::string("volume nbhood: alpha is 0 .. levels - 1");
            return std::string(nbhood.max_dist >= 1 && nbhood.max_dist <= MI_UNET_VNBHOOD_MAX_DIST ? "" : "volume nbhood: max_dist is 1 .. MI_UNET_VNBHOOD_MAX_DIST");
        },
        [&](std::ostream &lg, const Settings &) {
            lg << "Volume nbhood: " << quantiser_text(nbhood) << ", alpha " << nbhood.alpha << ", dist " << nbhood.max_dist;
        },
        /*handle_side=*/false);
}

bool set_volume_match(const VolumeMatch &match)
{
    return change_setting(
        [&](Settings &s) {
            s.volume_match = match;
            const bool ok = match.iou_num >= 1 && match.iou_num <= match.iou_den && match.iou_den <= 65536;
            return std::string(ok ? "" : "volume match: the threshold is 1 <= iou_num <= iou_den <= 65536");
        },
        [&](std::ostream &lg, const Settings &) {
            lg << "Volume match: " << (match.on ? "on" : "off") << ", iou " << match.iou_num << "/" << match.iou_den;
        },
        /*handle_side=*/false);
}

Settings current_settings()
{
    std::lock_guard<std::mutex> lk(g_state_mutex);
    return g_settings;
}
std::vector<Target> get_targets()
{
    std::vector<Target> out;
    for (const auto &x : current_settings().targets) out.push_back({ x.cls, x.min_area_frac });
    return out;
}
std::vector<Morph> get_morphology() { return current_settings().morph; }
mi_unet_window get_window() { return Preprocess::get_window(); }
mi_unet_measure get_measure() { return current_settings().measure; }
std::string get_truth_dir() { return current_settings().truth_dir; }
Volume get_volume() { return current_settings().volume; }
VolumeClean get_volume_clean() { return current_settings().volume_clean; }
VolumeMesh get_volume_mesh() { return current_settings().volume_mesh; }
VolumeInterp get_volume_interp() { return current_settings().volume_interp; }
VolumeMeasure get_volume_measure() { return current_settings().volume_measure; }
VolumeSpatial get_volume_spatial() { return current_settings().volume_spatial; }
VolumeSplit get_volume_split() { return current_settings().volume_split; }
VolumeSkeleton get_volume_skeleton() { return current_settings().volume_skeleton; }
VolumeBranches get_volume_branches() { return current_settings().volume_branches; }
VolumeTexture get_volume_texture() { return current_settings().volume_texture; }
VolumeZones get_volume_zones() { return current_settings().volume_zones; }
VolumeNbhood get_volume_nbhood() { return current_settings().volume_nbhood; }
VolumeMatch get_volume_match() { return current_settings().volume_match; }

std::ofstream &get_log_file() { return g_log_file; }
std::string get_log_path() { return g_log_path; }

int device_lanes(mi_unet_group_t *lanes[2], bool second)
{
    std::lock_guard<std::mutex> lk(g_state_mutex);
    if (!g_group) throw std::runtime_error("Engine not initialized");
    if (second && !g_lane2) {
        if (mi_unet_group_clone(g_group, &g_lane2) == MI_UNET_OK) {
            (void)g_settings.apply(g_lane2);                    // a clone starts at the defaults; the setters keep it current from here
        } else {
            if (g_log_file.is_open()) g_log_file << "Warning: second device lane unavailable (" << mi_unet_last_error() << ")" << std::endl;
            g_lane2 = nullptr;
        }
    }
    lanes[0] = g_group; lanes[1] = second ? g_lane2 : nullptr;
    return lanes[1] ? 2 : 1;
}

// The reference's get_thread_local_context() + initialize_context() (src/process.cpp:17-19, :45-120): the calling thread's
// own context, created on first use.
mi_unet_t *get_thread_local_context() { return thread_context(nullptr); }

mi_unet_t *thread_context(Settings *applied)
{
    std::lock_guard<std::mutex> lk(g_state_mutex);
    if (!g_group) throw std::runtime_error("Engine not initialized");
    if (!t_context.h || t_context.generation != g_generation) {
        t_context.release();
        if (mi_unet_clone(mi_unet_group_handle(g_group, 0), g_thread_batch, &t_context.h) != MI_UNET_OK)
            throw std::runtime_error(std::string("context creation failed: ") + mi_unet_last_error());
        t_context.generation = g_generation;
        std::lock_guard<std::mutex> ll(g_log_mutex);
        if (g_log_file.is_open())
            g_log_file << "Execution context created for a new thread (micro-batch " << g_thread_batch << ")" << std::endl;
    }
    // a clone starts at the defaults, and a setter may have run since this thread's last call (the values were validated when set)
    (void)g_settings.apply(t_context.h);
    if (applied) *applied = g_settings;
    return t_context.h;
}

namespace {
// single-plane tiles / RAW images feed every input channel of a multi-channel engine: the grey -> B,G,R replication of
// cv::imread(IMREAD_COLOR) (src/mask2polygon.cpp:117); see mi_unet_infer_raw16 in include/mi_unet.h
std::vector<uint8_t> interleave_gray(const std::vector<const Image8 *> &imgs, int in_ch)
{
    const size_t hw = (size_t)g_cfg.height * g_cfg.width;
    std::vector<uint8_t> in(hw * in_ch * imgs.size());
    for (size_t i = 0; i < imgs.size(); ++i) {
        const Image8 &g = *imgs[i];
        if (g.rows != g_cfg.height || g.cols != g_cfg.width || g.channels != 1)
            throw std::runtime_error("Input size must be " + std::to_string(g_cfg.width) + "x" + std::to_string(g_cfg.height) +
                                     " for fixed context");                                   // src/process.cpp:127
        uint8_t *dst = in.data() + i * hw * in_ch;
        if (in_ch == 1) std::copy(g.data.begin(), g.data.end(), dst);
        else
            for (size_t p = 0; p < hw; ++p)
                for (int c = 0; c < in_ch; ++c) dst[p * in_ch + c] = g.data[p];
    }
    return in;
}
}  // namespace

std::vector<Image8> execute_inference_batch(const std::vector<Image8> &gray_imgs)
{
    try {
        mi_unet_group_t *group = get_engine_group();
        if (!group) throw std::runtime_error("Engine not initialized");
        const size_t hw = (size_t)g_cfg.height * g_cfg.width;
        std::vector<const Image8 *> ptrs;
        for (const Image8 &g : gray_imgs) ptrs.push_back(&g);
        const std::vector<uint8_t> in = interleave_gray(ptrs, g_cfg.in_ch);
        std::vector<uint8_t> out(hw * gray_imgs.size());
        {
            std::lock_guard<std::mutex> lk(g_batch_mutex);
            if (mi_unet_group_infer_u8(group, in.data(), (int)gray_imgs.size(), out.data(), nullptr) != MI_UNET_OK)
                throw std::runtime_error(mi_unet_last_error());
        }
        std::vector<Image8> masks;
        for (size_t i = 0; i < gray_imgs.size(); ++i) masks.push_back(tile_image(out, i));
        return masks;
    } catch (const std::exception &e) {
        throw std::runtime_error("Inference failed: " + std::string(e.what()));               // src/process.cpp:173
    }
}

// One tile on the calling thread's own context (src/process.cpp:123-175).
Image8 execute_inference(const Image8 &gray_img)
{
    try {
        mi_unet_t *ctx = get_thread_local_context();
        const std::vector<uint8_t> in = interleave_gray({ &gray_img }, g_cfg.in_ch);
        Image8 mask(g_cfg.height, g_cfg.width, 1);
        if (mi_unet_infer_u8(ctx, in.data(), 1, mask.data.data(), nullptr) != MI_UNET_OK) throw std::runtime_error(mi_unet_last_error());
        return mask;
    } catch (const std::exception &e) {
        throw std::runtime_error("Inference failed: " + std::string(e.what()));               // src/process.cpp:173
    }
}

Image8 mask_to_image(const Image8 &mask)
{
    uint8_t lut[256] = { 0 };
    lut[1] = 128;
    lut[2] = 255;
    Image8 vis(mask.rows, mask.cols, 1);
    for (size_t i = 0; i < mask.data.size(); ++i) vis.data[i] = lut[mask.data[i]];
    return vis;
}

// Releases the calling thread's context (as the reference does, src/cleanup.cpp:16-35), the engine group and the log.
// Contexts of other threads notice the generation change and are released on their next use or when their thread ends
// (they share the weight blob, which lives until the last of them is gone).
void cleanup_resources()
{
    try {
        std::lock_guard<std::mutex> lk(g_state_mutex);
        if (g_log_file.is_open()) g_log_file << "\n=== Cleaning Up Resources ===" << std::endl;
        if (t_context.h) {
            t_context.release();
            if (g_log_file.is_open()) g_log_file << "Execution context destroyed" << std::endl;
        }
        ++g_generation;
        release_pinned_buffers();
        if (g_lane2) { mi_unet_group_destroy(g_lane2); g_lane2 = nullptr; }
        if (g_group) {
            mi_unet_group_destroy(g_group);         // every device's buffers, streams, worker thread, weights
            g_group = nullptr;
            if (g_log_file.is_open()) g_log_file << "MI355X UNet engine destroyed" << std::endl;
        }
        if (g_log_file.is_open()) {
            g_log_file << "All resources cleaned up successfully" << std::endl;
            g_log_file.close();
        }
        std::cout << "Resources cleaned up successfully" << std::endl;
    } catch (const std::exception &e) {
        std::cerr << "Cleanup error: " << e.what() << std::endl;
    }
}

}  // namespace MedicalSeg
