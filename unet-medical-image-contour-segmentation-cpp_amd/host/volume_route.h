// volume_route.h -- what routes.cpp and volume_route.cpp share: the stack that a batch fills with the slices of one volume, the chain
// that runs behind its last device call, and the small helpers both files write their log lines and reports with.  Private to host/.
#pragma once
#include <chrono>
#include <ostream>
#include <stdexcept>
#include <string>
#include <vector>

#include "facade.h"

namespace MedicalSeg {

using hr_clock = std::chrono::high_resolution_clock;
inline long long ms_since(hr_clock::time_point t0) { return std::chrono::duration_cast<std::chrono::milliseconds>(hr_clock::now() - t0).count(); }

// (routes.cpp) a failure of one image, one batch or one step of the volume chain: on stderr and in the log
void report(std::ostream &lg, const std::string &msg);
// (routes.cpp) a double as JSON: %.17g, null when it is not finite
std::string json_number(double v);

// One stage of include/mi_unet.h that has a form on a handle and a `_host` form with the same arguments behind it: the device form on
// `h`, or the host form under MEDSEG_HOST_POSTPROCESS=1 and without a handle.  stage_rc returns the code; stage_call throws the
// library's message when it is not MI_UNET_OK, and checked does the same for a function of one form (_derive, _units, _assign).
template <class OnDevice, class OnHost, class... Args>
int stage_rc(mi_unet_t *h, OnDevice on_device, OnHost on_host, Args... args)
{
    return (h && device_postprocess_requested()) ? on_device(h, args...) : on_host(args...);
}
template <class Fn, class... Args>
void checked(Fn fn, Args... args)
{
    if (fn(args...) != MI_UNET_OK) throw std::runtime_error(mi_unet_last_error());
}
template <class OnDevice, class OnHost, class... Args>
void stage_call(mi_unet_t *h, OnDevice on_device, OnHost on_host, Args... args)
{
    if (stage_rc(h, on_device, on_host, args...) != MI_UNET_OK) throw std::runtime_error(mi_unet_last_error());
}

// ---- set_volume: the images of a batch as the slices of one volume.  process_images_targets fills the stack as its images finish;
// finish_volume runs once, behind the last device call of the batch.
struct VolumeStack {
    // `s` decides what the stack keeps beside the planes: with set_volume_measure on, its channel of every slice's normalised tile; with
    // set_volume_texture on, its channel likewise, in a stack of its own only when the two channels differ; with set_volume_zones on, its
    // channel, in a stack of its own only when neither of the other two holds it; with set_volume_nbhood on, its channel, in a stack of
    // its own only when none of the other three holds it; with set_volume_spatial on, its channel, in a stack of its own only when none of
    // the other four holds it
    VolumeStack(size_t slices, size_t hw, const Settings &s)
        : channel(s.volume_measure.on ? s.volume_measure.channel : -1), texture_channel(s.volume_texture.on ? s.volume_texture.channel : -1),
          zones_channel(s.volume_zones.on ? s.volume_zones.channel : -1), nbhood_channel(s.volume_nbhood.on ? s.volume_nbhood.channel : -1),
          spatial_channel(s.volume_spatial.on ? s.volume_spatial.channel : -1),
          planes(s.targets.size() * slices * hw, 0), intensity(channel >= 0 ? slices * hw : 0, 0),
          texture_own(texture_channel >= 0 && texture_channel != channel ? slices * hw : 0, 0),
          zones_own(zones_channel >= 0 && zones_channel != channel && zones_channel != texture_channel ? slices * hw : 0, 0),
          nbhood_own(nbhood_channel >= 0 && nbhood_channel != channel && nbhood_channel != texture_channel && nbhood_channel != zones_channel
                         ? slices * hw
                         : 0,
                     0),
          spatial_own(spatial_channel >= 0 && spatial_channel != channel && spatial_channel != texture_channel && spatial_channel != zones_channel &&
                              spatial_channel != nbhood_channel
                          ? slices * hw
                          : 0,
                      0),
          bases(slices), names(slices), D(slices), hw(hw)
    {
    }
    // image i of the batch is complete: plane t of its K final 0 / 255 pictures becomes slice i of target t; `tile` is its normalised
    // tile, [H][W][C]
    void add(size_t i, const std::string &base, const uint8_t *pictures, size_t K, const uint8_t *tile, size_t C)
    {
        for (size_t t = 0; t < K; ++t) std::copy(pictures + t * hw, pictures + (t + 1) * hw, planes.begin() + (t * D + i) * hw);
        if (channel >= 0 && (size_t)channel < C)
            for (size_t p = 0; p < hw; ++p) intensity[i * hw + p] = tile[p * C + (size_t)channel];
        if (!texture_own.empty() && (size_t)texture_channel < C)
            for (size_t p = 0; p < hw; ++p) texture_own[i * hw + p] = tile[p * C + (size_t)texture_channel];
        if (!zones_own.empty() && (size_t)zones_channel < C)
            for (size_t p = 0; p < hw; ++p) zones_own[i * hw + p] = tile[p * C + (size_t)zones_channel];
        if (!nbhood_own.empty() && (size_t)nbhood_channel < C)
            for (size_t p = 0; p < hw; ++p) nbhood_own[i * hw + p] = tile[p * C + (size_t)nbhood_channel];
        if (!spatial_own.empty() && (size_t)spatial_channel < C)
            for (size_t p = 0; p < hw; ++p) spatial_own[i * hw + p] = tile[p * C + (size_t)spatial_channel];
        bases[i] = base;
    }
    const uint16_t *texture_intensity() const { return texture_own.empty() ? intensity.data() : texture_own.data(); }
    const uint16_t *zones_intensity() const
    {
        return !zones_own.empty() ? zones_own.data() : zones_channel == channel ? intensity.data() : texture_intensity();
    }
    const uint16_t *nbhood_intensity() const
    {
        return !nbhood_own.empty() ? nbhood_own.data() : nbhood_channel == zones_channel ? zones_intensity() : nbhood_channel == channel ? intensity.data() : texture_intensity();
    }
    const uint16_t *spatial_intensity() const
    {
        return !spatial_own.empty() ? spatial_own.data() : spatial_channel == nbhood_channel ? nbhood_intensity() : spatial_channel == zones_channel ? zones_intensity() : spatial_channel == channel ? intensity.data() : texture_intensity();
    }
    int channel, texture_channel, zones_channel, nbhood_channel, spatial_channel;      // -1: not kept
    std::vector<uint8_t> planes;                       // [K][D][H][W]; a slice that failed stays all-zero
    std::vector<uint16_t> intensity;                   // [D][H][W] or empty: the measured channel of the normalised tiles, widened
    std::vector<uint16_t> texture_own;                 // [D][H][W] or empty: the texture's channel where it is not the measured one
    std::vector<uint16_t> zones_own;                   // [D][H][W] or empty: the zones' channel where neither of the two above holds it
    std::vector<uint16_t> nbhood_own;                  // [D][H][W] or empty: the neighbourhoods' channel where none of the three above holds it
    std::vector<uint16_t> spatial_own;                 // [D][H][W] or empty: the spatial statistics' channel where none of the four above holds it
    std::vector<std::string> bases, names;             // per slice: the base name once it is complete (else empty); the name it is reported by
    size_t D, hw;
};

// (volume_route.cpp) The chain behind the last device call of a volume batch, every stage on `h` (its host form under
// MEDSEG_HOST_POSTPROCESS=1): clean_volume when set_volume_clean is on -- its failure ends the chain -- then label_volume with whatever
// of interpolation, mesh, measure, texture, zones, neighbourhoods and spatial statistics is on, then score_volume_stack with a truth directory, and in it match_volume when set_volume_match is on.
// A failure of a step is reported to `lg` and fails no image.
void finish_volume(VolumeStack &stack, const Settings &s, mi_unet_t *h, const std::string &output_dir, std::ostream &lg);

}  // namespace MedicalSeg
