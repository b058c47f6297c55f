// volume_mesh.hip -- the border of one value plane of a mask stack as oriented quads over shared vertices (include/mi_unet.h:
// mi_unet_volume_mesh).  Two counting kernels (one lane per voxel, one lane per grid corner) leave a count per
// workgroup; a hierarchical exclusive scan turns the counts into output bases; two emitting kernels write every vertex and every quad
// at base + rank inside the workgroup, the rank from ballots.  No output position depends on the arrival order of an atomic, and no
// workgroup waits for another.  Byte and integer work, exact.  gfx950 only.
#include "../../include/mi_unet.h"
#include "kernel_common.h"
#include "kernels.h"
#include "wave.h"

namespace miunet {

namespace vm {

using namespace wave;

constexpr unsigned WG = 256;                // lanes per workgroup of the voxel and corner kernels
constexpr unsigned CHUNK = 1024;            // counts one workgroup of the scan takes: four per lane

inline size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }
inline unsigned blocks(unsigned n) { return (n + WG - 1) / WG; }
inline unsigned chunks(unsigned n) { return (n + CHUNK - 1) / CHUNK; }

// ints behind the first level of a scan of n counts: the sums of every level above it
inline size_t scan_sums(unsigned n)
{
    size_t total = 0;
    while (n > 1) {
        n = chunks(n);
        total += up256(n);
    }
    return total + 256;
}

// The workspace of one plane.  qtot / vtot hold one count per workgroup of the voxel / corner kernels and one entry more, zeroed: behind
// the exclusive scan that entry is the total.  The levels of the scan lie behind each.
struct Ws {
    uint8_t *expo;                  // [dhw] the voxel's exposure mask, bit d = direction d (-x, +x, -y, +y, -z, +z)
    int *cmap;                      // [nc] per grid corner: the vertex's (ox, oy, oz, n) as its last four bytes, 0 = no vertex; then its index
    int *qtot, *vtot;
    unsigned dhw, nc, nbq, nbc;
    size_t total;
};

inline Ws carve(void *base, int D, int H, int W)
{
    uint8_t *p = static_cast<uint8_t *>(base);
    Ws w;
    w.dhw = (unsigned)D * (unsigned)H * (unsigned)W;
    w.nc = (unsigned)(D + 1) * (unsigned)(H + 1) * (unsigned)(W + 1);
    w.nbq = blocks(w.dhw);
    w.nbc = blocks(w.nc);
    size_t at = 0;
    w.expo = p + at; at += up256(w.dhw);
    w.cmap = reinterpret_cast<int *>(p + at); at += up256((size_t)w.nc * sizeof(int));
    w.qtot = reinterpret_cast<int *>(p + at); at += (up256(w.nbq + 1) + scan_sums(w.nbq + 1)) * sizeof(int);
    w.vtot = reinterpret_cast<int *>(p + at); at += (up256(w.nbc + 1) + scan_sums(w.nbc + 1)) * sizeof(int);
    w.total = at;
    return w;
}

// ---- classify: one lane per voxel, consecutive lanes along x ------------------------------------------------------------------------------
// The six neighbours are read straight from the volume: a row's x neighbours lie in the lane's own cache line, the rows above and below
// and the two neighbouring slices are the lines the workgroups beside this one read, so the volume leaves HBM about once.  The per-axis
// counts of a lane are at most 2 each; packed ten bits apart a workgroup's sums (at most 512) cannot meet.
__global__ __launch_bounds__(256) void k_vm_classify(const uint8_t *__restrict__ masks, int v, int D, int H, int W, unsigned dhw,
                                                     uint8_t *__restrict__ expo, int *__restrict__ qtot, unsigned long long *axis)
{
    __shared__ int s_w[4];
    const unsigned i = blockIdx.x * WG + threadIdx.x;
    int m = 0;
    if (i < dhw) {
        if (masks[i] == v) {
            const unsigned hw = (unsigned)H * (unsigned)W;
            const int z = (int)(i / hw), rem = (int)(i - (unsigned)z * hw), y = rem / W, x = rem - y * W;
            const uint8_t *const p = masks + i;
            if (x == 0 || p[-1] != v) m |= 1;
            if (x == W - 1 || p[1] != v) m |= 2;
            if (y == 0 || p[-W] != v) m |= 4;
            if (y == H - 1 || p[W] != v) m |= 8;
            if (z == 0 || p[-(long long)hw] != v) m |= 16;
            if (z == D - 1 || p[hw] != v) m |= 32;
        }
        expo[i] = (uint8_t)m;
    }
    const int t = wave_offsets(wave_sum(__popc(m & 3) | (__popc(m & 12) << 10) | (__popc(m & 48) << 20)), s_w).y;
    if (threadIdx.x == 0) {
        const int cx = t & 1023, cy = (t >> 10) & 1023, cz = (t >> 20) & 1023;
        qtot[blockIdx.x] = cx + cy + cz;
        if (cx) atomicAdd(axis + 0, (unsigned long long)cx);
        if (cy) atomicAdd(axis + 1, (unsigned long long)cy);
        if (cz) atomicAdd(axis + 2, (unsigned long long)cz);
    }
}

// ---- corners: one lane per grid corner, consecutive lanes along x ---------------------------------------------------------------------------
// bit (dz * 4 + dy * 2 + dx) of `in` = voxel (i - 1 + dx, j - 1 + dy, k - 1 + dz) is in the set.  The twelve edges of the 2 x 2 x 2
// block join positions that differ in one of dx, dy, dz: the cut ones are the set bits of in ^ (in shifted by that axis) at the
// positions with the axis bit clear.
__device__ __forceinline__ int corner_word(int in, int placement)
{
    if (in == 0 || in == 255) return 0;                         // no edge is cut: the edge graph of the block is connected
    if (placement == VOLUME_MESH_FACES) return 1 << 24;
    const int cutx = (in ^ (in >> 1)) & 0x55, cuty = (in ^ (in >> 2)) & 0x33, cutz = (in ^ (in >> 4)) & 0x0F;
    const int n = __popc(cutx) + __popc(cuty) + __popc(cutz);
    // an edge's midpoint is at +1 on another axis where its position has that axis' bit set, else at -1
    const int ox = 2 * (__popc(cuty & 0xAA & 0x33) + __popc(cutz & 0xAA & 0x0F)) - __popc(cuty) - __popc(cutz);
    const int oy = 2 * (__popc(cutx & 0xCC & 0x55) + __popc(cutz & 0xCC & 0x0F)) - __popc(cutx) - __popc(cutz);
    const int oz = 2 * (__popc(cutx & 0xF0 & 0x55) + __popc(cuty & 0xF0 & 0x33)) - __popc(cutx) - __popc(cuty);
    return (ox & 255) | ((oy & 255) << 8) | ((oz & 255) << 16) | (n << 24);
}

__global__ __launch_bounds__(256) void k_vm_corners(const uint8_t *__restrict__ masks, int v, int placement, int D, int H, int W, unsigned nc,
                                                    int *__restrict__ cmap, int *__restrict__ vtot)
{
    __shared__ int s_w[4];
    const unsigned c = blockIdx.x * WG + threadIdx.x;
    int word = 0;
    if (c < nc) {
        const unsigned w1 = (unsigned)W + 1u, h1 = (unsigned)H + 1u;
        const unsigned t = c / w1;
        const int i = (int)(c - t * w1), j = (int)(t % h1), k = (int)(t / h1);
        int in = 0;
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const int x = i - 1 + (b & 1), y = j - 1 + ((b >> 1) & 1), z = k - 1 + (b >> 2);
            if (x >= 0 && x < W && y >= 0 && y < H && z >= 0 && z < D && masks[((size_t)z * H + y) * W + x] == v) in |= 1 << b;
        }
        word = corner_word(in, placement);
        cmap[c] = word;
    }
    const int n = wave_offsets(__popcll(__ballot(word != 0)), s_w).y;
    if (threadIdx.x == 0) vtot[blockIdx.x] = n;
}

// ---- scan: exclusive, in place, CHUNK counts per workgroup; the workgroup's sum goes to sums[blockIdx.x] ------------------------------------
__global__ __launch_bounds__(256) void k_vm_scan_chunk(int *__restrict__ a, unsigned n, int *__restrict__ sums)
{
    __shared__ int s_w[4];
    const unsigned base = blockIdx.x * CHUNK + threadIdx.x * 4u;
    int v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = base + j < n ? a[base + j] : 0;
    const int own = v[0] + v[1] + v[2] + v[3];
    int x = own;                                                // inclusive over the wave
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(x, o, 64);
        if (lane >= o) x += t;
    }
    const int2 off = wave_offsets(__shfl(x, 63, 64), s_w);
    int run = off.x + x - own;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (base + j < n) a[base + j] = run;
        run += v[j];
    }
    if (threadIdx.x == 0 && sums) sums[blockIdx.x] = off.y;
}

__global__ __launch_bounds__(256) void k_vm_scan_add(int *__restrict__ a, unsigned n, const int *__restrict__ sums)
{
    const unsigned i = blockIdx.x * WG + threadIdx.x;
    if (i < n) a[i] += sums[i / CHUNK];
}

__global__ void k_vm_totals(const int *q, const int *v, unsigned long long *counts)
{
    if (threadIdx.x == 0) {
        counts[0] = (unsigned long long)*q;
        counts[1] = (unsigned long long)*v;
    }
}

// ---- emit ----------------------------------------------------------------------------------------------------------------------------------
// A corner's vertex index = the vertices of the workgroups before it (vbase) + of the waves before it + of the lanes below it.
__global__ __launch_bounds__(256) void k_vm_emit_verts(int *__restrict__ cmap, const int *__restrict__ vbase, int H, int W, unsigned nc,
                                                       int4 *__restrict__ verts, int keep)
{
    __shared__ int s_w[4];
    const unsigned c = blockIdx.x * WG + threadIdx.x;
    const int word = c < nc ? cmap[c] : 0;
    const unsigned long long b = __ballot(word != 0);
    const int2 off = wave_offsets(__popcll(b), s_w);
    if (!word) return;
    const int rank = vbase[blockIdx.x] + off.x + __popcll(b & lanes_below());
    if (rank < keep) {
        const unsigned w1 = (unsigned)W + 1u, h1 = (unsigned)H + 1u;
        const unsigned t = c / w1;
        verts[rank] = make_int4((int)(c - t * w1), (int)(t % h1), (int)(t / h1), word);
    }
    cmap[c] = rank;
}

// A voxel's first quad = the quads of the workgroups before it (qbase) + of the waves before it + of the lanes below it; its own follow
// in the order of the directions.  Corner offsets of direction d relative to the voxel's corner (x, y, z), include/mi_unet.h ORIENTATION.
__global__ __launch_bounds__(256) void k_vm_emit_quads(const uint8_t *__restrict__ expo, const int *__restrict__ qbase,
                                                       const int *__restrict__ cmap, int H, int W, unsigned dhw, int4 *__restrict__ quads, int keep)
{
    __shared__ int s_w[4];
    const int first = qbase[blockIdx.x];
    if (first >= keep) return;                                  // (the whole workgroup: nothing of it is kept)
    const unsigned i = blockIdx.x * WG + threadIdx.x;
    const int m = i < dhw ? expo[i] : 0;
    const unsigned long long below = lanes_below();
    int before = 0, total = 0;
#pragma unroll
    for (int d = 0; d < 6; ++d) {
        const unsigned long long b = __ballot((m >> d) & 1);
        before += __popcll(b & below);
        total += __popcll(b);
    }
    const int2 off = wave_offsets(total, s_w);
    if (!m) return;
    int rank = first + off.x + before;
    const unsigned hw = (unsigned)H * (unsigned)W;
    const int z = (int)(i / hw), rem = (int)(i - (unsigned)z * hw), y = rem / W, x = rem - y * W;
    const int sy = W + 1, sz = (H + 1) * (W + 1);
    const int *const c0 = cmap + ((size_t)z * (H + 1) + y) * (W + 1) + x;
    // per direction the four corners, three bits (dx, dy, dz) each, first corner in the low bits
    constexpr int CORNERS[6] = {
        0 | (4 << 3) | (6 << 6) | (2 << 9), 1 | (3 << 3) | (7 << 6) | (5 << 9),
        0 | (1 << 3) | (5 << 6) | (4 << 9), 2 | (6 << 3) | (7 << 6) | (3 << 9),
        0 | (2 << 3) | (3 << 6) | (1 << 9), 4 | (5 << 3) | (7 << 6) | (6 << 9) };
#pragma unroll
    for (int d = 0; d < 6; ++d) {
        if (!((m >> d) & 1)) continue;
        if (rank < keep) {
            int q[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int bits = (CORNERS[d] >> (3 * j)) & 7;
                q[j] = c0[(bits & 1) + ((bits >> 1) & 1) * sy + (bits >> 2) * sz];
            }
            quads[rank] = make_int4(q[0], q[1], q[2], q[3]);
        }
        ++rank;
    }
}

// exclusive scan of a[0 .. n) in place; `sums` = the levels above it (scan_sums(n) ints)
void scan(int *a, unsigned n, int *sums, hipStream_t s)
{
    const unsigned nb = chunks(n);
    hipLaunchKernelGGL(k_vm_scan_chunk, dim3(nb), dim3(WG), 0, s, a, n, nb > 1 ? sums : nullptr);
    if (nb > 1) {
        scan(sums, nb, sums + up256(nb), s);
        hipLaunchKernelGGL(k_vm_scan_add, dim3(blocks(n)), dim3(WG), 0, s, a, n, sums);
    }
}

bool fits(const VolumeMeshArgs &a)
{
    if (a.D < 1 || a.H < 1 || a.W < 1) return false;
    long long v = 0x7FFFFFFFLL / 6;                             // 6 (D + 1) (H + 1) (W + 1) < 2^31, step by step
    v /= (long long)a.D + 1;
    v /= (long long)a.H + 1;
    return v >= (long long)a.W + 1;
}

}  // namespace vm

size_t volume_mesh_workspace_bytes(int D, int H, int W) { return vm::carve(nullptr, D, H, W).total; }

hipError_t launch_volume_mesh_count(const uint8_t *masks, const VolumeMeshArgs &a, unsigned long long *counts, void *ws, hipStream_t s)
{
    if (!masks || !counts || !ws || !vm::fits(a) || a.value < 0 || a.value > 255) return hipErrorInvalidValue;
    if (a.placement != VOLUME_MESH_FACES && a.placement != VOLUME_MESH_NETS) return hipErrorInvalidValue;
    const vm::Ws w = vm::carve(ws, a.D, a.H, a.W);
    if (hipError_t e = hipMemsetAsync(counts, 0, 5 * sizeof(unsigned long long), s)) return e;
    if (hipError_t e = hipMemsetAsync(w.qtot + w.nbq, 0, sizeof(int), s)) return e;
    if (hipError_t e = hipMemsetAsync(w.vtot + w.nbc, 0, sizeof(int), s)) return e;
    hipLaunchKernelGGL(vm::k_vm_classify, dim3(w.nbq), dim3(vm::WG), 0, s, masks, a.value, a.D, a.H, a.W, w.dhw, w.expo, w.qtot, counts + 2);
    hipLaunchKernelGGL(vm::k_vm_corners, dim3(w.nbc), dim3(vm::WG), 0, s, masks, a.value, a.placement, a.D, a.H, a.W, w.nc, w.cmap, w.vtot);
    vm::scan(w.qtot, w.nbq + 1, w.qtot + vm::up256(w.nbq + 1), s);
    vm::scan(w.vtot, w.nbc + 1, w.vtot + vm::up256(w.nbc + 1), s);
    hipLaunchKernelGGL(vm::k_vm_totals, dim3(1), dim3(64), 0, s, w.qtot + w.nbq, w.vtot + w.nbc, counts);
    return hipGetLastError();
}

hipError_t launch_volume_mesh_emit(const VolumeMeshArgs &a, void *ws, ::mi_unet_mesh_vertex *verts, int keep_verts, int32_t *quads,
                                   int keep_quads, hipStream_t s)
{
    if (!ws || !vm::fits(a) || keep_verts < 0 || keep_quads < 0 || (!verts && keep_verts) || (!quads && keep_quads)) return hipErrorInvalidValue;
    static_assert(sizeof(::mi_unet_mesh_vertex) == sizeof(int4), "a vertex is stored as one int4");
    const vm::Ws w = vm::carve(ws, a.D, a.H, a.W);
    if (!keep_verts && !keep_quads) return hipSuccess;
    hipLaunchKernelGGL(vm::k_vm_emit_verts, dim3(w.nbc), dim3(vm::WG), 0, s, w.cmap, w.vtot, a.H, a.W, w.nc, reinterpret_cast<int4 *>(verts),
                       keep_verts);
    if (keep_quads)
        hipLaunchKernelGGL(vm::k_vm_emit_quads, dim3(w.nbq), dim3(vm::WG), 0, s, w.expo, w.qtot, w.cmap, a.H, a.W, w.dhw,
                           reinterpret_cast<int4 *>(quads), keep_quads);
    return hipGetLastError();
}

}  // namespace miunet
