// window.cpp -- the intensity window of the RAW-in entry points (include/mi_unet.h: mi_unet_set_window): the setting,
// its definition as host arithmetic (mi_unet_window_of), and what pipeline_raw.cpp and pipeline_tiled.cpp share: the (lo, hi) slot
// of every plane of a call, the scratch of the device selection and the report behind mi_unet_last_windows.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "engine_handle.h"

namespace miunet {

int check_window(const mi_unet_window &w, const char *fn)
{
    const std::string f = fn;
    switch (w.mode) {
    case MI_UNET_WINDOW_MINMAX:
        return MI_UNET_OK;
    case MI_UNET_WINDOW_PERCENTILE:
        if (w.clip_lo_ppm < 0 || w.clip_hi_ppm < 0 || (long long)w.clip_lo_ppm + w.clip_hi_ppm >= 1000000)
            return fail(MI_UNET_EARG, f + ": percentile window needs clip_lo_ppm >= 0, clip_hi_ppm >= 0 and their sum below 1000000 (got " +
                                          std::to_string(w.clip_lo_ppm) + ", " + std::to_string(w.clip_hi_ppm) + ")");
        return MI_UNET_OK;
    case MI_UNET_WINDOW_FIXED:
        if (!(0 <= w.lo && w.lo < w.hi && w.hi <= 65535))
            return fail(MI_UNET_EARG, f + ": fixed window needs 0 <= lo < hi <= 65535 (got " + std::to_string(w.lo) + ", " + std::to_string(w.hi) + ")");
        return MI_UNET_OK;
    default:
        return fail(MI_UNET_EARG, f + ": unknown window mode " + std::to_string(w.mode));
    }
}

int begin_window_call(mi_unet *h, size_t planes, size_t scratch_planes, unsigned long long max_samples, const std::string &fn)
{
    const mi_unet_window &w = h->window;
    if (w.mode == MI_UNET_WINDOW_PERCENTILE && max_samples >= (1ull << 32))
        return fail(MI_UNET_EARG, fn + ": a percentile window counts in 32 bits: planes of 2^32 samples or more are not supported");
    h->last_win_valid = false;
    h->win_src.assign(planes, 0);
    for (size_t i = 0; i < planes; ++i) h->win_src[i] = (int)i;
    // nothing of an earlier call is in flight here (every RAW-in call drains its streams before it returns)
    if (planes > h->win_cap) {
        const size_t cap = std::max(planes, (size_t)h->cfg.max_batch * h->cfg.in_ch);
        h->win_cap = 0;
        HIP_TRY(h->d_mnmx.reset(2 * cap));
        HIP_TRY(h->h_win.reset(2 * cap));
        h->win_cap = cap;
    }
    if (w.mode == MI_UNET_WINDOW_PERCENTILE && scratch_planes > h->win_ws_slots) {
        h->win_ws_slots = 0;
        HIP_TRY(h->d_win_ws.reset(scratch_planes * window_scratch_bytes()));
        h->win_ws_slots = scratch_planes;
    }
    return 0;
}

hipError_t enqueue_window(mi_unet *h, const uint16_t *d_raw, size_t n, size_t slot, size_t ws_slot, hipStream_t s)
{
    const mi_unet_window &w = h->window;
    if (slot >= h->win_cap) return hipErrorInvalidValue;
    if (w.mode == MI_UNET_WINDOW_MINMAX) return launch_minmax_u16(d_raw, n, h->d_mnmx + 2 * slot, s);
    if (w.mode == MI_UNET_WINDOW_FIXED) return hipSuccess;
    if (ws_slot >= h->win_ws_slots) return hipErrorInvalidValue;
    uint8_t *ws = h->d_win_ws + ws_slot * window_scratch_bytes();
    if (hipError_t e = hipMemsetAsync(ws, 0, window_scratch_bytes(), s)) return e;
    return launch_window_select_u16(d_raw, n, w.clip_lo_ppm, w.clip_hi_ppm, ws, h->d_mnmx + 2 * slot, s);
}

int enqueue_window_download(mi_unet *h, size_t planes, hipStream_t s)
{
    if (h->window.mode == MI_UNET_WINDOW_FIXED || planes == 0) return 0;
    HIP_TRY(hipMemcpyAsync(h->h_win, h->d_mnmx, sizeof(unsigned) * 2 * planes, hipMemcpyDeviceToHost, s));
    return 0;
}

void finish_window_call(mi_unet *h, size_t planes)
{
    h->last_win.resize(2 * planes);
    for (size_t i = 0; i < planes; ++i) {
        const size_t src = (size_t)h->win_src[i];
        const bool fixed = h->window.mode == MI_UNET_WINDOW_FIXED;
        h->last_win[2 * i] = fixed ? h->window.lo : (int32_t)h->h_win[2 * src];
        h->last_win[2 * i + 1] = fixed ? h->window.hi : (int32_t)h->h_win[2 * src + 1];
    }
    h->last_win_valid = true;
}

}  // namespace miunet

using namespace miunet;

extern "C" {

int mi_unet_set_window(mi_unet_t *h, const mi_unet_window *w)
{
    if (int rc = check_handle(h, false)) return rc;
    const mi_unet_window nw = w ? *w : kDefaultWindow;
    if (int rc = check_window(nw, "mi_unet_set_window")) return rc;
    h->window = nw;
    return MI_UNET_OK;
}

int mi_unet_get_window(const mi_unet_t *h, mi_unet_window *w)
{
    if (!h || !w) return fail(MI_UNET_EARG, "mi_unet_get_window: null argument");
    *w = h->window;
    return MI_UNET_OK;
}

int mi_unet_window_of(const uint16_t *samples, size_t n, const mi_unet_window *w, int *lo, int *hi)
{
    if (!samples || n == 0 || !lo || !hi) return fail(MI_UNET_EARG, "mi_unet_window_of: null argument or no samples");
    const mi_unet_window win = w ? *w : kDefaultWindow;
    if (int rc = check_window(win, "mi_unet_window_of")) return rc;
    if (win.mode == MI_UNET_WINDOW_FIXED) {
        *lo = win.lo; *hi = win.hi;
        return MI_UNET_OK;
    }
    // the definition in histogram terms: the smallest value whose cumulative count exceeds the rank
    std::vector<unsigned long long> hist(65536, 0);
    for (size_t i = 0; i < n; ++i) ++hist[samples[i]];
    const bool pct = win.mode == MI_UNET_WINDOW_PERCENTILE;
    const unsigned long long k_lo = pct ? (unsigned long long)n * (unsigned)win.clip_lo_ppm / 1000000ull : 0;
    const unsigned long long k_hi = pct ? (unsigned long long)n * (unsigned)win.clip_hi_ppm / 1000000ull : 0;
    const unsigned long long rank[2] = { k_lo, (unsigned long long)n - 1 - k_hi };
    int out[2] = { 0, 0 };
    unsigned long long cum = 0;
    int r = 0;
    for (int v = 0; v < 65536 && r < 2; ++v) {
        cum += hist[v];
        while (r < 2 && cum > rank[r]) out[r++] = v;
    }
    *lo = out[0]; *hi = out[1];
    return MI_UNET_OK;
}

int mi_unet_last_windows(const mi_unet_t *h, int32_t *lo_hi, int cap, int *n)
{
    if (!h || !n || cap < 0 || (cap > 0 && !lo_hi)) return fail(MI_UNET_EARG, "mi_unet_last_windows: bad argument");
    if (!h->last_win_valid) return fail(MI_UNET_ESTATE, "mi_unet_last_windows: no RAW-in call has completed on this handle");
    const int count = (int)(h->last_win.size() / 2);
    *n = count;
    std::copy(h->last_win.begin(), h->last_win.begin() + 2 * (size_t)std::min(count, cap), lo_hi);
    return MI_UNET_OK;
}

}  // extern "C"
