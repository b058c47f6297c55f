// tile_grid.h -- the overlap-tile grid of the tiled entry points (mi_unet_infer_tiled_*, include/mi_unet.h): which tiles cover an
// image axis and which output positions each of them owns.  Pure integer arithmetic, shared by the host (pipeline_tiled.cpp, the
// exported mi_unet_tile_axis) and the kernels of tiles.hip, and free of any device API so that a host-only test can include it
// (tests/cpu/tile_axis_test.cpp).  Internal to libmiunet.so.
//
// One axis of length L, tile length T, halo h (L >= T, h >= 0, 2h < T):
//   S   = T - 2h                       stride of tile origins
//   n   = 1 + ceil((L - T) / S)        tiles
//   o_k = min(k S, L - T)              origin of tile k: the last tile ends at the image edge
//   c_0 = 0, c_n = L, c_k = (o_{k-1} + T + o_k) / 2      tile k owns [c_k, c_{k+1})
// A cut is the middle of the overlap of two neighbouring tiles, and neighbouring tiles overlap by at least 2h, so every owned
// position lies at least h inside every tile border that is not an image border.
#pragma once

#if defined(__HIPCC__)
#define MIUNET_HD __host__ __device__
#else
#define MIUNET_HD
#endif

namespace miunet {

MIUNET_HD inline bool tile_axis_ok(int L, int T, int halo) { return T > 0 && L >= T && halo >= 0 && 2 * (long long)halo < T; }

MIUNET_HD inline int tile_count(int L, int T, int halo)
{
    const int S = T - 2 * halo;
    return 1 + (L - T + S - 1) / S;
}

MIUNET_HD inline int tile_origin(int L, int T, int S, int k)
{
    const long long o = (long long)k * S;
    return o < L - T ? (int)o : L - T;
}

// cut k of n tiles, k = 0..n
MIUNET_HD inline int tile_cut(int L, int T, int S, int n, int k)
{
    if (k <= 0) return 0;
    if (k >= n) return L;
    return (int)(((long long)tile_origin(L, T, S, k - 1) + T + tile_origin(L, T, S, k)) / 2);
}

// the tiles whose extent [o_k, o_k + T) holds position pos (0 <= pos < L) are exactly first .. last (blending)
MIUNET_HD inline int tile_first_cover(int T, int S, int pos) { return pos < T ? 0 : (pos - T) / S + 1; }
MIUNET_HD inline int tile_last_cover(int L, int T, int S, int n, int pos) { return pos >= L - T ? n - 1 : pos / S; }

// mirror averaging (mirror = MI_UNET_MIRROR_X | MI_UNET_MIRROR_Y bits, 0..3): the views of one tile, in the order identity, X (if
// bit 0), Y (if bit 1), XY (if both); view v's own flips as the same bits (1: columns reversed, 2: rows reversed)
MIUNET_HD inline int tile_view_count(int mirror) { return mirror == 3 ? 4 : mirror ? 2 : 1; }
MIUNET_HD inline int tile_view_flip(int mirror, int v) { return mirror == 3 ? v : v ? mirror : 0; }

// origins[n] and cuts[n + 1] (either may be null); returns n, or -1 for an illegal (L, T, halo)
inline int tile_axis(int L, int T, int halo, int *origins, int *cuts)
{
    if (!tile_axis_ok(L, T, halo)) return -1;
    const int S = T - 2 * halo, n = tile_count(L, T, halo);
    for (int k = 0; k < n && origins; ++k) origins[k] = tile_origin(L, T, S, k);
    for (int k = 0; k <= n && cuts; ++k) cuts[k] = tile_cut(L, T, S, n, k);
    return n;
}

// The grid of one image as the kernels take it (by value): tile t = ty * nx + tx
struct TileGrid {
    int H, W;             // image
    int th, tw;           // tile
    int sy, sx;           // origin strides
    int ny, nx;
};

inline bool tile_grid(int H, int W, int th, int tw, int halo, TileGrid &g)
{
    if (!tile_axis_ok(H, th, halo) || !tile_axis_ok(W, tw, halo)) return false;
    g.H = H; g.W = W; g.th = th; g.tw = tw;
    g.sy = th - 2 * halo; g.sx = tw - 2 * halo;
    g.ny = tile_count(H, th, halo); g.nx = tile_count(W, tw, halo);
    return true;
}

}  // namespace miunet
