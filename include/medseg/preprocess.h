// Reference: include/preprocess.h:20-23, src/preprocess.cpp:76-141.
#pragma once
#include <cstdint>
#include <memory>
#include <string>
#include <vector>

#include "../mi_unet.h"
#include "image.h"

namespace Preprocess {

// mmap the headerless little-endian u16 RAW (w*h*2 bytes), min/max, top-left-aligned bilinear resample to 512x512 in
// double, quantise to u8, write the PNG (level 0) and the one-line size JSON.  false on failure.
bool preprocess_raw(const std::string &raw_path, const std::string &png_path, const std::string &json_path, int w, int h);

// Pieces of the above, exposed so the device-first pipeline can reuse them: the checked mmap read of the RAW file, and the
// PNG (level 0) + one-line size JSON writers (src/preprocess.cpp:121-134).
std::vector<uint16_t> read_raw16(const std::string &raw_path, int w, int h);
// Under a non-default intensity window (below) the size JSON gains "window_hi" and "window_lo", the window applied to the image:
// `lo_hi` when given, else the window in force evaluated on the RAW file itself (window_of -- the definition the device meets).
bool write_preprocess_outputs(const medseg::Image8 &tile, const std::string &raw_path, const std::string &png_path,
                              const std::string &json_path, int w, int h, const int *lo_hi = nullptr);

// Read-only view of the RAW file -- the checked mmap itself (file length and MAP_FAILED verified, sizes in size_t; the
// reference's MMapFile, src/preprocess.cpp:28-61, checks neither).  The device-first pipeline copies from it straight into
// pinned staging memory: one copy between the page cache and the GPU.  Throws std::runtime_error.
class RawView {
public:
    RawView(const std::string &raw_path, int w, int h);
    const uint16_t *data() const { return static_cast<const uint16_t *>(map_.get()); }
    size_t samples() const { return samples_; }

private:
    std::shared_ptr<void> map_;
    size_t samples_ = 0;
};

// The arithmetic of the above on memory (no files): src/preprocess.cpp:81-118.
medseg::Image8 resample_normalize(const uint16_t *src, int w, int h, int outW = 512, int outH = 512);

// Intensity windows (mi_unet_window in include/mi_unet.h) -- the same arithmetic on the CPU:
//   window_of                 : (lo, hi) of n samples under `win` (mi_unet_window_of); false for a setting the engine would refuse
//   resample_normalize_window : resample_normalize with the interpolant clamped to lo .. max(hi, lo + 1) and stretched onto 0 .. 255
//   set_window / get_window   : the process-wide window that preprocess_raw and write_preprocess_outputs apply
//                               (MedicalSeg::set_window keeps it equal to the engine's); the default is the min/max stretch
bool window_of(const uint16_t *src, size_t n, const mi_unet_window &win, int &lo, int &hi);
medseg::Image8 resample_normalize_window(const uint16_t *src, int w, int h, int lo, int hi, int outW = 512, int outH = 512);
bool set_window(const mi_unet_window &win);
mi_unet_window get_window();

}  // namespace Preprocess
