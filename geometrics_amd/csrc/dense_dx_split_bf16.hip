// The first layer's input gradient dX = G . W^T ([rows, 192] x [192, cin], cin = 963 / 1155) on the BF16 matrix cores with EXACT
// fp32 products (the arithmetic of dense_split_bf16.hip: fp32 = bf16 + bf16 + bf16 exactly, products of two bf16 numbers are
// exact in fp32, the six terms with i + j <= 2, the leading term g0 w0 in one fp32 accumulator and the five small ones in a
// second one, added once at the end).
//
// Why this product and not the forward one: the summed index is only 192, so a workgroup's share of G stays on
// chip for the whole launch.  A workgroup owns up to 6 consecutive 16-row blocks of G (1281 row-blocks over 256 workgroups:
// 5 or 6 each, one round, no stray tile); its prologue splits them ONCE into three bf16 planes in LDS (<= 96 x 192 x 2 B x 3 =
// 108 KB).  W is split once per call by a small launch of its own, into planes stored IN FRAGMENT ORDER: the 36 KB a wave
// needs for one group of DX_NT column tiles are contiguous, and every 16-byte-per-lane load of it is one contiguous KB.
// A wave holds the B fragments of a column group for all of K in registers (DX_NT x 3 planes x 6 k-blocks x 4 VGPRs), sweeps
// the workgroup's row-blocks reading A fragments with ds_read_b128, and stores each finished 16 x (16 DX_NT) piece while
// the next row-block's MFMAs run.  The B registers exist twice: the NEXT group's fragments are requested in equal shares
// during the row-blocks of the current group -- every workgroup pulls all 1.1 MB of planes through its L2 port once, which
// at the ~70 GB/s a CU gets from L2 takes about as long as its MFMAs, so that stream has to run all the time, not in bursts.
// The sweep is compiled once per row-block count (1 .. 6) as straight-line code, so that every wait for a B fragment is
// counted against the stores issued since (the memory counter is in order; a wait in front of a loop would drain them).
// The four waves take column groups wave, wave + 4, ...
//
// Every output element is hi + lo with hi = sum over the six k-blocks, ascending, of g0 w0 and lo the same sum of the five
// small terms in a fixed order: a function of its own row of G and its own row of W only -- bit-reproducible, and the same
// whichever workgroup, tile or launch computes the row.
//
// Probe builds (tools/probe/dx_variants.sh; never the product): -DDX_PROBE_NO_STORE, -DDX_PROBE_NO_LDS, -DDX_PROBE_NO_REFILL,
// -DDX_PROBE_NO_PROLOGUE take one stream out of the launch each (results are then wrong; the MFMAs stay: the stores hang on a
// condition the compiler cannot see through).
#include "buffer_access.h"
#include "device_facts.h"
#include <type_traits>

namespace {

using namespace geom;

constexpr int DX_THREADS = 256;
constexpr int DX_K = 192;                       // the summed index (the layer width)
constexpr int DX_KB = DX_K / 32;                // k-blocks of one MFMA
constexpr int DX_NT = 2;                        // 16-column tiles a wave keeps register-stationary
constexpr int DX_MAX_RB = 6;                    // 16-row blocks of G a workgroup keeps in LDS
constexpr int DX_ROW_BYTES = DX_K * 2;          // one row of one plane: 384 B = 24 chunks of 16 B
constexpr int DX_PLANE = DX_MAX_RB * 16 * DX_ROW_BYTES;   // 36 864 B
constexpr int DX_LDS = 3 * DX_PLANE;            // 110 592 B

// a -> (a0, a1, a2) as bf16 bit patterns, a0 + a1 + a2 == a exactly for finite a below the last bf16 binade.  The conversion is
// the compiler's cast (v_cvt_pk_bf16_f32), NOT integer rounding of the fp32 bits: a NaN stays a NaN in every plane (the
// integer form turns some NaNs into zeros), an infinity splits into inf + NaN + NaN.
__device__ __forceinline__ unsigned bf16_bits_of(float x) { return (unsigned)__builtin_bit_cast(unsigned short, (__bf16)x); }
__device__ __forceinline__ float bf16_value_of(unsigned bits) { return __uint_as_float(bits << 16); }
__device__ __forceinline__ void split3(float a, unsigned &b0, unsigned &b1, unsigned &b2)
{
    b0 = bf16_bits_of(a);
    const float r1 = a - bf16_value_of(b0);
    b1 = bf16_bits_of(r1);
    const float r2 = r1 - bf16_value_of(b1);
    b2 = bf16_bits_of(r2);
}

// Fragment order of the planes: element (column, k, plane) sits at
//   ((((group * 6 + kb) * DX_NT + t) * 3 + plane) * 64 + lane) * 8 + j
// with group = column / (16 DX_NT), t = column / 16 % DX_NT, kb = k / 32, lane = 16 (k / 8 % 4) + column % 16, j = k % 8:
// lane (lr, lg) of a wave reads its B fragment of (group, kb, t, plane) -- w_plane[column 16 (DX_NT group + t) + lr][k = 32 kb +
// 8 lg .. + 7] -- as 16 bytes, the wave 1 KB, a whole group 36 KB in the order the sweep uses it.
__host__ __device__ __forceinline__ size_t dx_frag_index(int group, int kb, int t, int plane, int lane)
{
    return ((((size_t)group * DX_KB + kb) * DX_NT + t) * 3 + plane) * 64 + lane;      // in 16-byte fragments
}

// planes of w [cin][192] fp32 (columns cin .. cinpad - 1 zero): thread = one (column, 8 consecutive k) = one fragment per plane
__global__ __launch_bounds__(256) void dx_planes_kernel(int cin, int cinpad, const float *w, uint4 *planes)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= cinpad * (DX_K / 8)) return;
    const int col = i / (DX_K / 8), k8 = i - col * (DX_K / 8);
    unsigned e[8][3];
#pragma unroll
    for (int j = 0; j < 8; ++j) e[j][0] = e[j][1] = e[j][2] = 0;
    if (col < cin) {
        const float4 lo = *reinterpret_cast<const float4 *>(w + (size_t)col * DX_K + 8 * k8);
        const float4 hi = *reinterpret_cast<const float4 *>(w + (size_t)col * DX_K + 8 * k8 + 4);
        const float v[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
#pragma unroll
        for (int j = 0; j < 8; ++j) split3(v[j], e[j][0], e[j][1], e[j][2]);
    }
    const int tile = col >> 4;
#pragma unroll
    for (int pl = 0; pl < 3; ++pl)
        planes[dx_frag_index(tile / DX_NT, k8 >> 2, tile % DX_NT, pl, 16 * (k8 & 3) + (col & 15))] =
            make_uint4(e[0][pl] | (e[1][pl] << 16), e[2][pl] | (e[3][pl] << 16), e[4][pl] | (e[5][pl] << 16), e[6][pl] | (e[7][pl] << 16));
}

// Every global access of the product is a buffer access against one of three descriptors (g, the planes, dx; each below
// 2 GiB, the host checks); an access that must not happen gets the offset OOB (buffer_access.h), so every load and store is
// issued on every path and the waits below can count them.

struct DxArgs {
    const float *g;              // [rows][192] fp32, 16-byte aligned
    const void *wp;              // the planes in fragment order (dx_frag_index)
    float *dx;                   // [rows][cin] at a pitch of ldx floats
    int rows, cin, cinpad, ldx, spread;
};

// LDS image of one plane: row r (of the workgroup's tile) at r * 384 B, its 16-byte chunk q (k = 8 q .. 8 q + 7) at chunk
// q ^ ((r >> 1) & 7): the 16 lanes ds_read_b128 serves in one cycle (eight rows of one k group, eight of the next) then cover
// sixteen different 16-byte slots of the 256-byte bank row
__device__ __forceinline__ int lds_chunk(int r, int q) { return r * DX_ROW_BYTES + ((q ^ ((r >> 1) & 7)) << 4); }

// One k-block of one row-block: the six terms, per term the tiles in turn (an accumulator is touched every DX_NT-th MFMA).
// THE order of the sum of every output element: hi takes g0 w0, lo takes g0 w1, g1 w0, g1 w1, g0 w2, g2 w0.
__device__ __forceinline__ void dx_terms(const bf16x8 (&a)[3], const bf16x8 (&b)[DX_NT][3], f32x4 (&hi)[DX_NT], f32x4 (&lo)[DX_NT])
{
#pragma unroll
    for (int t = 0; t < DX_NT; ++t) hi[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[0], b[t][0], hi[t], 0, 0, 0);
#pragma unroll
    for (int t = 0; t < DX_NT; ++t) lo[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[0], b[t][1], lo[t], 0, 0, 0);
#pragma unroll
    for (int t = 0; t < DX_NT; ++t) lo[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[1], b[t][0], lo[t], 0, 0, 0);
#pragma unroll
    for (int t = 0; t < DX_NT; ++t) lo[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[1], b[t][1], lo[t], 0, 0, 0);
#pragma unroll
    for (int t = 0; t < DX_NT; ++t) lo[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[0], b[t][2], lo[t], 0, 0, 0);
#pragma unroll
    for (int t = 0; t < DX_NT; ++t) lo[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[2], b[t][0], lo[t], 0, 0, 0);
}

// hi + lo of row-block `rb` (of the matrix) x column group `grp` to dX.  D layout of the 16 x 16 tile: column = lane & 15, row =
// 4 (lane >> 4) + register; rows of dX are 4-byte aligned only, so dword stores (64-byte pieces of four rows each)
__device__ __forceinline__ void dx_store(const DxArgs &p, __amdgpu_buffer_rsrc_t r_dx, int rb, int grp, int lane, const f32x4 (&hi)[DX_NT],
                                         const f32x4 (&lo)[DX_NT])
{
    const int row = rb * 16 + 4 * (lane >> 4), col = grp * (16 * DX_NT) + (lane & 15);
#pragma unroll
    for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int t = 0; t < DX_NT; ++t) {
            const unsigned off = row + e < p.rows && col + 16 * t < p.cin ? (unsigned)(((row + e) * p.ldx + col + 16 * t) * 4) : OOB;
#ifdef DX_PROBE_NO_STORE
            if (p.ldx < 0)
#endif
            __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(hi[t][e] + lo[t][e]), r_dx, off, 0, 0);
        }
}

// The sweep of a workgroup with N row-blocks in LDS (rows rb0 * 16 ..): straight-line code over the row-blocks of two
// consecutive column groups of the wave (B register sets 0 and 1 in turn).
template <int N>
__device__ __forceinline__ void dx_sweep(const DxArgs &p, const unsigned char *lds, int wave, int lane, int rb0)
{
    const int lr = lane & 15, lg = lane >> 4;      // fragment coordinates: row / column lr, k group lg (8 consecutive k)
    const int ngroups = p.cinpad / (16 * DX_NT);
    bf16x8 bf[2][DX_KB][DX_NT][3];
    bf16x8 af[2][3];
    const __amdgpu_buffer_rsrc_t r_w = rsrc(p.wp, (int64_t)3 * p.cinpad * DX_K * 2);
    const __amdgpu_buffer_rsrc_t r_dx = rsrc(p.dx, ((int64_t)(p.rows - 1) * p.ldx + p.cin) * 4);
    // A fragments of (row-block, k-block): lane (lr, lg) holds g_plane[row 16 rbi + lr][k = 32 kb + 8 lg .. + 7].  Two register sets
    // in turn: the fragments of the next k-block (after the last one: of the next row-block's first) are requested in front of
    // this k-block's MFMAs -- one wave per SIMD has nobody else to cover an LDS read
    auto a_frags = [&](int set, int rbi, int kb) {
#pragma unroll
        for (int pl = 0; pl < 3; ++pl)
            af[set][pl] = *reinterpret_cast<const bf16x8 *>(lds + pl * DX_PLANE + lds_chunk(rbi * 16 + lr, 4 * kb + lg));
    };
    auto b_frags = [&](int set, int grp, int kb) {      // (a group beyond the last: nothing is fetched)
        const unsigned base = grp < ngroups ? (unsigned)(dx_frag_index(grp, 0, 0, 0, lane) * 16) : OOB;
#pragma unroll
        for (int t = 0; t < DX_NT; ++t)
#pragma unroll
            for (int pl = 0; pl < 3; ++pl)
                bf[set][kb][t][pl] = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(r_w, base + (unsigned)(dx_frag_index(0, kb, t, pl, 0) * 16), 0, 0));
    };
    // one column group on B set `set`; group `next` follows it on the other set, whose k-blocks are requested in N shares
    auto group = [&](auto set_c, int grp, int next) {
        constexpr int S = decltype(set_c)::value;
#pragma unroll
        for (int rbi = 0; rbi < N; ++rbi) {
            f32x4 hi[DX_NT], lo[DX_NT];
#pragma unroll
            for (int t = 0; t < DX_NT; ++t) hi[t] = lo[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
#ifndef DX_PROBE_NO_REFILL
#pragma unroll
            for (int kb = rbi * DX_KB / N; kb < (rbi + 1) * DX_KB / N; ++kb) b_frags(S ^ 1, next, kb);
#endif
#pragma unroll
            for (int kb = 0; kb < DX_KB; ++kb) {
                const int s = kb & 1;
#ifndef DX_PROBE_NO_LDS
                if (kb + 1 < DX_KB) a_frags(s ^ 1, rbi, kb + 1);
                else a_frags(0, rbi + 1 < N ? rbi + 1 : 0, 0);
                __builtin_amdgcn_sched_barrier(0);      // (the scheduler otherwise sinks each read to just in front of its MFMA)
#endif
                dx_terms(af[s], bf[S][kb], hi, lo);
            }
            dx_store(p, r_dx, rb0 + rbi, grp, lane, hi, lo);
        }
    };

    if (wave >= ngroups) return;
#pragma unroll
    for (int kb = 0; kb < DX_KB; ++kb) b_frags(0, wave, kb);
#ifdef DX_PROBE_NO_REFILL
#pragma unroll
    for (int kb = 0; kb < DX_KB; ++kb) b_frags(1, wave, kb);
#endif
    a_frags(0, 0, 0);
    for (int grp = wave; grp < ngroups; grp += 8) {
        group(std::integral_constant<int, 0>(), grp, grp + 4);
        if (grp + 4 < ngroups) group(std::integral_constant<int, 1>(), grp + 4, grp + 8);
    }
}

// A stray row-block (LDS row-block `lds_rb`, row-block `rb` of the matrix) against ONE column group: what is left of the rows
// when they do not divide over the workgroups is spread, a group each, over workgroups -- whose wave 3 has a group less than the
// others to do -- instead of giving one workgroup a row-block more (1281 = 5 x 256 + 1: a sixth of the launch).
__device__ __forceinline__ void dx_stray(const DxArgs &p, const unsigned char *lds, int lane, int lds_rb, int rb, int grp)
{
    const int lr = lane & 15, lg = lane >> 4;
    const __amdgpu_buffer_rsrc_t r_w = rsrc(p.wp, (int64_t)3 * p.cinpad * DX_K * 2);
    const __amdgpu_buffer_rsrc_t r_dx = rsrc(p.dx, ((int64_t)(p.rows - 1) * p.ldx + p.cin) * 4);
    bf16x8 b[DX_KB][DX_NT][3];
#pragma unroll
    for (int kb = 0; kb < DX_KB; ++kb)
#pragma unroll
        for (int t = 0; t < DX_NT; ++t)
#pragma unroll
            for (int pl = 0; pl < 3; ++pl)
                b[kb][t][pl] = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(r_w, (unsigned)(dx_frag_index(grp, kb, t, pl, lane) * 16), 0, 0));
    f32x4 hi[DX_NT], lo[DX_NT];
#pragma unroll
    for (int t = 0; t < DX_NT; ++t) hi[t] = lo[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kb = 0; kb < DX_KB; ++kb) {
        bf16x8 a[3];
#pragma unroll
        for (int pl = 0; pl < 3; ++pl) a[pl] = *reinterpret_cast<const bf16x8 *>(lds + pl * DX_PLANE + lds_chunk(lds_rb * 16 + lr, 4 * kb + lg));
        dx_terms(a, b[kb], hi, lo);
    }
    dx_store(p, r_dx, rb, grp, lane, hi, lo);
}

__global__ __launch_bounds__(DX_THREADS, 1) void dx_split_kernel(DxArgs p)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int nrb = (p.rows + 15) >> 4;
    // the workgroup's row-blocks rb0 .. rb0 + n - 1 (n = 1 .. DX_MAX_RB: the host sizes the grid) and, with p.spread, for the first
    // workgroups one column group of a stray row-block behind the equal shares
    int rb0 = (int)((int64_t)blockIdx.x * nrb / gridDim.x), n = (int)((int64_t)(blockIdx.x + 1) * nrb / gridDim.x) - rb0;
    int stray_rb = -1, stray_grp = 0;
    if (p.spread) {
        const int ngroups = p.cinpad / (16 * DX_NT), share = nrb / (int)gridDim.x;
        rb0 = blockIdx.x * share, n = share;
        if ((int)blockIdx.x < (nrb - share * (int)gridDim.x) * ngroups) stray_rb = share * gridDim.x + blockIdx.x / ngroups, stray_grp = blockIdx.x % ngroups;
    }

    // ---- prologue: the workgroup's rows of G, split once into three planes in LDS (rows beyond the matrix: zeros).  All loads
    // first (one HBM round trip for the tile, not one per piece), then the split
#ifndef DX_PROBE_NO_PROLOGUE
    {
        const __amdgpu_buffer_rsrc_t r_g = rsrc(p.g, (int64_t)p.rows * DX_K * 4);
        u32x4 v[3 * DX_MAX_RB];
#pragma unroll
        for (int i = 0; i < 3 * DX_MAX_RB; ++i) {      // piece q = tid + 256 i: row q / 48 of the tile, floats 4 (q % 48) ..
            const int q = tid + DX_THREADS * i, r = q / (DX_K / 4);
            const int row = r < 16 * n ? rb0 * 16 + r : stray_rb * 16 + r - 16 * n;      // (the stray block: LDS row-block n)
            const unsigned off = r < 16 * n || (stray_rb >= 0 && r < 16 * n + 16) ? (unsigned)((row * DX_K + 4 * (q - r * (DX_K / 4))) * 4) : OOB;
            v[i] = __builtin_amdgcn_raw_buffer_load_b128(r_g, off, 0, 0);
        }
#pragma unroll
        for (int i = 0; i < 3 * DX_MAX_RB; ++i) {
            const int q = tid + DX_THREADS * i, r = q / (DX_K / 4), c4 = q - r * (DX_K / 4);
            unsigned e[4][3];
            split3(__uint_as_float(v[i].x), e[0][0], e[0][1], e[0][2]);
            split3(__uint_as_float(v[i].y), e[1][0], e[1][1], e[1][2]);
            split3(__uint_as_float(v[i].z), e[2][0], e[2][1], e[2][2]);
            split3(__uint_as_float(v[i].w), e[3][0], e[3][1], e[3][2]);
            unsigned char *dst = lds + lds_chunk(r, c4 >> 1) + 8 * (c4 & 1);
#pragma unroll
            for (int pl = 0; pl < 3; ++pl)
                *reinterpret_cast<uint2 *>(dst + pl * DX_PLANE) = make_uint2(e[0][pl] | (e[1][pl] << 16), e[2][pl] | (e[3][pl] << 16));
        }
    }
#endif
    __syncthreads();
    switch (n) {
    case 1: dx_sweep<1>(p, lds, wave, lane, rb0); break;
    case 2: dx_sweep<2>(p, lds, wave, lane, rb0); break;
    case 3: dx_sweep<3>(p, lds, wave, lane, rb0); break;
    case 4: dx_sweep<4>(p, lds, wave, lane, rb0); break;
    case 5: dx_sweep<5>(p, lds, wave, lane, rb0); break;
    case 6: dx_sweep<6>(p, lds, wave, lane, rb0); break;
    default: break;
    }
    if (stray_rb >= 0 && wave == 3) dx_stray(p, lds, lane, n, stray_rb, stray_grp);
}

} // namespace

// rows of the planes buffer: cin rounded up to whole column groups of a wave
extern "C" int geom_dense_dx_split_cinpad(int cin) { return cin <= 0 ? 0 : (cin + 16 * DX_NT - 1) / (16 * DX_NT) * (16 * DX_NT); }

// planes (3 x cinpad x 192 bf16 in fragment order, see dx_frag_index) <- w [cin][192] fp32: w == plane 0 + plane 1 + plane 2
// exactly, padding columns zero
extern "C" int geom_dense_dx_split_planes_f32(int cin, int c, const float *w, uint16_t *planes, void *stream)
{
    if (cin <= 0 || c <= 0) return GEOM_EINVAL;
    if (c != DX_K) return GEOM_EUNSUPPORTED;
    if (!w || !planes || ((uintptr_t)w & 15) || ((uintptr_t)planes & 15)) return GEOM_EINVAL;
    const int cinpad = geom_dense_dx_split_cinpad(cin);
    if ((int64_t)cinpad * DX_K * 6 >= (1LL << 31)) return GEOM_ETOOBIG;
    const int frags = cinpad * (DX_K / 8);
    hipLaunchKernelGGL(dx_planes_kernel, dim3((unsigned)((frags + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), cin, cinpad, w,
                       reinterpret_cast<uint4 *>(planes));
    return geom::launch_status();
}

// dx [rows, cin] (row pitch ldx >= cin floats) = g [rows, 192] . w^T with w [cin, 192] given as planes (geom_dense_dx_split_planes_f32)
extern "C" int geom_dense_dx_split_f32(int rows, int cin, int c, const float *g, const uint16_t *planes, float *dx, int ldx, void *stream)
{
    if (rows < 0 || cin <= 0 || c <= 0 || ldx < cin) return GEOM_EINVAL;
    if (c != DX_K) return GEOM_EUNSUPPORTED;
    if (rows == 0) return 0;
    if (!g || !planes || !dx || ((uintptr_t)g & 15) || ((uintptr_t)planes & 15) || ((uintptr_t)dx & 3)) return GEOM_EINVAL;
    const int cinpad = geom_dense_dx_split_cinpad(cin);
    // (32-bit byte offsets against descriptors below 2 GiB)
    if ((int64_t)cinpad * DX_K * 6 >= (1LL << 31) || (int64_t)rows * ldx * 4 >= (1LL << 31) || (int64_t)rows * DX_K * 4 >= (1LL << 31)) return GEOM_ETOOBIG;
    DxArgs p{g, planes, dx, rows, cin, cinpad, ldx, 0};
    const geom::DeviceFacts *dev = geom::device_facts();
    if (int code = geom::allow_dynamic_lds(dx_split_kernel, DX_LDS, dev)) return code;
    // whole rounds of one workgroup per compute unit, each with at most DX_MAX_RB row-blocks, as evenly as they divide
    const int64_t nrb = ((int64_t)rows + 15) >> 4;
    const int64_t cus = dev ? dev->compute_units : 256;
    const int64_t rounds = (nrb + DX_MAX_RB * cus - 1) / (DX_MAX_RB * cus);
    const int64_t grid = nrb < rounds * cus ? nrb : rounds * cus;
    // what the equal shares leave over (fewer row-blocks than workgroups) goes out a column group each, where there are
    // workgroups enough for that (the kernel's stray role); otherwise some workgroups get a row-block more
    const int64_t left = nrb % grid;
    p.spread = left > 0 && left * (cinpad / (16 * DX_NT)) <= grid;
    hipLaunchKernelGGL(dx_split_kernel, dim3((unsigned)grid), dim3(DX_THREADS), DX_LDS, static_cast<hipStream_t>(stream), p);
    return geom::launch_status();
}
