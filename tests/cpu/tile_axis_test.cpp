// CPU test of the overlap-tile grid (csrc/tile_grid.h), host only: the header's per-tile functions (what the kernels of tiles.hip
// evaluate per lane) against tile_axis' arrays and against the definition written out again here, and a whole-image check that
// the owned rectangles of a 2-D grid partition the image.  Prints one line per failure; exit code 0 = all passed.
#include <algorithm>
#include <cstdio>
#include <vector>

#include "../../unet-medical-image-contour-segmentation-cpp_amd/csrc/tile_grid.h"

using namespace miunet;

static int failures = 0;
static long checks = 0;
#define CHECK(cond, ...) do { ++checks; if (!(cond)) { ++failures; std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)

int main()
{
    // 1. one axis: the definition, restated
    for (int T : { 16, 24, 40, 64, 512 })
        for (int h = 0; 2 * h < T && h <= 40; ++h)
            for (int L = T; L <= 5 * T + 2; ++L) {
                const int S = T - 2 * h;
                int n = 1;
                while ((n - 1) * S < L - T) ++n;                             // 1 + ceil((L - T) / S)
                std::vector<int> o(n + 8, -7), c(n + 9, -7);
                const int got = tile_axis(L, T, h, o.data(), c.data());
                CHECK(got == n, "L=%d T=%d h=%d: n=%d, expected %d", L, T, h, got, n);
                if (got != n) continue;
                CHECK(o[n] == -7 && c[n + 1] == -7, "L=%d T=%d h=%d: wrote past n", L, T, h);
                CHECK(tile_count(L, T, h) == n, "tile_count");
                for (int k = 0; k < n; ++k) {
                    const int ok = std::min(k * S, L - T);
                    CHECK(o[k] == ok && tile_origin(L, T, S, k) == ok, "L=%d T=%d h=%d: origin %d = %d, expected %d", L, T, h, k, o[k], ok);
                }
                for (int k = 0; k <= n; ++k) {
                    const int ck = k == 0 ? 0 : k == n ? L : (std::min((k - 1) * S, L - T) + T + std::min(k * S, L - T)) / 2;
                    CHECK(c[k] == ck && tile_cut(L, T, S, n, k) == ck, "L=%d T=%d h=%d: cut %d = %d, expected %d", L, T, h, k, c[k], ck);
                }
                for (int k = 0; k < n; ++k) {
                    CHECK(c[k] < c[k + 1], "L=%d T=%d h=%d: empty ownership of tile %d", L, T, h, k);
                    CHECK(o[k] <= c[k] && c[k + 1] <= o[k] + T, "L=%d T=%d h=%d: tile %d owns outside itself", L, T, h, k);
                    if (k > 0) CHECK(c[k] - o[k] >= h, "L=%d T=%d h=%d: tile %d left margin %d", L, T, h, k, c[k] - o[k]);
                    if (k < n - 1) CHECK(o[k] + T - c[k + 1] >= h, "L=%d T=%d h=%d: tile %d right margin %d", L, T, h, k, o[k] + T - c[k + 1]);
                }
            }
    // 2. illegal arguments, null outputs
    CHECK(tile_axis(15, 16, 0, nullptr, nullptr) == -1, "L < T");
    CHECK(tile_axis(64, 16, -1, nullptr, nullptr) == -1, "halo < 0");
    CHECK(tile_axis(64, 16, 8, nullptr, nullptr) == -1, "2 halo == T");
    CHECK(tile_axis(64, 0, 0, nullptr, nullptr) == -1, "T == 0");
    CHECK(tile_axis(64, 16, 7, nullptr, nullptr) == 25, "S = 2: 1 + 48 / 2 tiles");
    CHECK(tile_axis(16, 16, 7, nullptr, nullptr) == 1, "L == T");
    // 3. a 2-D grid: every pixel is owned by exactly one tile, numbered row-major
    for (int halo : { 0, 3, 11 }) {
        const int H = 100, W = 72, th = 40, tw = 24;
        TileGrid g{};
        CHECK(tile_grid(H, W, th, tw, halo, g), "tile_grid");
        std::vector<int> owner(H * W, -1);
        for (int t = 0; t < g.ny * g.nx; ++t) {
            const int ty = t / g.nx, tx = t % g.nx;
            for (int y = tile_cut(H, th, g.sy, g.ny, ty); y < tile_cut(H, th, g.sy, g.ny, ty + 1); ++y)
                for (int x = tile_cut(W, tw, g.sx, g.nx, tx); x < tile_cut(W, tw, g.sx, g.nx, tx + 1); ++x) {
                    CHECK(owner[y * W + x] == -1, "pixel (%d, %d) owned twice", x, y);
                    owner[y * W + x] = t;
                }
        }
        CHECK(std::find(owner.begin(), owner.end(), -1) == owner.end(), "halo %d: a pixel has no owner", halo);
    }
    if (failures == 0) std::printf("all %ld tile grid checks passed\n", checks);
    return failures ? 1 : 0;
}
