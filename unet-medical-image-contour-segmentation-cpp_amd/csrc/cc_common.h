// cc_common.h -- what image_stages.hip and regions.hip share: the lock-free union-find forest of the connected-component labelling
// and the layout of the contour stage's workspace.  Internal to libmiunet.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace miunet {
namespace pp {

__device__ __forceinline__ int ld(const int *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void st(int *p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// root of x with path halving: every store writes an ancestor of the node, so racing finds / unions stay consistent
__device__ __forceinline__ int find_root(int *parent, int x)
{
    int p = ld(parent + x);
    while (p != x) {
        const int g = ld(parent + p);
        if (g != p) st(parent + x, g);
        x = p; p = g;
    }
    return x;
}

// read-only walk for the flatten pass: there every store must be the final root, so no halving stores may race with it
__device__ __forceinline__ int find_root_ro(const int *parent, int x)
{
    for (int p = ld(parent + x); p != x; p = ld(parent + x)) x = p;
    return x;
}

// parents only ever decrease, roots satisfy parent[r] == r; atomicMin at L2 makes concurrent unions safe
__device__ __forceinline__ void unite(int *parent, int a, int b)
{
    for (;;) {
        a = find_root(parent, a);
        b = find_root(parent, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }          // a > b: hang a under b
        const int old = atomicMin(parent + a, b);
        if (old == a) return;
        a = old;                                                // somebody re-parented a meanwhile: retry from there
    }
}

}  // namespace pp

// The contour stage's workspace (contour_workspace_bytes) for B planes of H x W, n = B * H * W.  Seven n-int arrays: the two forests,
// `flag` (cc_init's area array: the reaches-the-frame flag of the background roots) and the four bounding-box arrays of cc_init,
// which the contour path never reads.  Behind the second cc_init every entry of `slot` (its minx array) is REGION_NO_SLOT; the
// measuring half (regions.hip) writes the contour index of every measured component at its root there.
constexpr int REGION_NO_SLOT = 0x7FFFFFFF;
struct ContourWs {
    int *fparent, *bparent, *flag, *slot, *miny, *maxx, *maxy;
    uint8_t *fg, *bg;               // the thresholded mask (255 / 0) and its complement
    int *roots, *npts, *counts;     // [B][cap_contours] sorted start pixels, their point counts; [B] external components found
};
inline ContourWs contour_ws(void *ws, long long n, int B, int cap_contours)
{
    ContourWs w;
    w.fparent = static_cast<int *>(ws); w.bparent = w.fparent + n; w.flag = w.bparent + n; w.slot = w.flag + n; w.miny = w.slot + n;
    w.maxx = w.miny + n; w.maxy = w.maxx + n;
    w.fg = reinterpret_cast<uint8_t *>(w.maxy + n); w.bg = w.fg + n;
    w.roots = reinterpret_cast<int *>(w.bg + n + ((16 - (2 * n) % 16) % 16));
    w.npts = w.roots + (size_t)B * cap_contours; w.counts = w.npts + (size_t)B * cap_contours;
    return w;
}

}  // namespace miunet
