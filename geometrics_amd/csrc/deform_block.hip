// A hidden layer of the mesh deformation block in ONE launch per direction (reference models.py:237-297
// with layers.py:107-116): the block follows every 0N-GCN layer with BatchNorm1d(verts) + ReLU, and every second one with the
// residual average `(features + x) / 2`.  As separate operators a hidden layer is three launches each way at the reference's
// training shape (16 meshes x 482 vertices = 7 712 rows, 192 wide): product 9.3 us, aggregation 7.3 us, per-vertex
// BatchNorm 6-7 us (profiles/r05_driver_step_timeline.txt), every one of them a latency chain on a mostly idle chip, with the
// 5.9 MB activation written and re-read between them.
//
//   forward  (geom_deform_layer_fwd_f32), one workgroup per VERTEX v, its B <= 16 batch rows = one 16-row MFMA tile:
//       Z   = [A . S[:, :64] | S[:, 64:]] + bias          the layer's aggregation (zn_gcn.hip's order: same bits)
//       X'  = ReLU(BatchNorm_v(Z))  (+ residual, * scale)  statistics over the vertex's B * 192 values: tile-local
//       S'  = X' . W_next                                  the NEXT layer's product, exact fp32 on v_mfma_f32_16x16x4_f32
//     writes Z (the BatchNorm backward needs it), X' (the next layer's weight gradient and the residuals need it), S'.
//   backward (geom_deform_layer_bwd_f32), same tiling:
//       G   = [A^T . dZ_up[:, :64] | dZ_up[:, 64:]]        aggregation backward of the layer ABOVE (written: its dW needs it)
//       dX  = G . W_up^T  (+ a second upstream gradient)   its input-gradient product
//       dZ  = BatchNorm_v backward (ReLU mask, residual scale) of THIS layer: the two reductions are tile-local again
//     writes G, dZ, the residual's gradient, the BatchNorm parameter gradients and the vertex's bias-gradient column sums.
//
// Why this tiling: BatchNorm1d(verts) normalises a vertex over (batch, channel), so the natural tile is "all batch rows of one
// vertex" -- exactly M = 16 of the fp32 MFMA -- and the only cross-tile dependencies of a layer are the two gathers
// (neighbours' support rows forward, neighbours' dZ rows backward), which is where the launch boundaries sit.  The weight
// operand is the row-block product's of mfma_tiles.h (zn_stack.hip runs the same one): a wave owns 48 output columns and holds
// its 192 x 48 slice in 144 registers, requested at kernel start so that it lands under the gather round trips; the activation
// tile goes through that product's LDS panel, one ds_read_b128 per 12 MFMAs.  482 workgroups of 4 waves, two resident per CU: while one
// waits for its gathers the other runs its 144 MFMAs per wave.
//
// Three tilings run the SAME layer: one row tile per vertex (db_fwd_body / db_bwd_body: the launches per layer and the chain
// launches), up to four tiles per vertex (dbw_fwd_kernel / dbw_bwd_kernel) and 16 consecutive rows of [b * nv] (di_row_block:
// eval; dp_fwd_row_block / dp_bwd_row_block: the BatchNorm-free block of the old driver).  The layer's steps -- a table row's
// unpacking, bias, BatchNorm + ReLU + residual, the statistics and their publication, the coordinate head both ways, the staging
// tile's way out, the BatchNorm backward, the column sums -- are stated once, as the db_* helpers around db_to_panel, and every
// body calls them: the wide route must give the one-tile route's bits, the eval route vertex_bn's.  The three row-block kernels
// share the dealing of row-blocks to workgroups (db_deal_row_blocks) and the host's grid (db_launch_row_blocks), the two plain
// ones their gather (db_row_aggregate).
// What stays apart, and why: the SCHEDULES differ on purpose -- the one-tile body requests the weight slice inside
// db_aggregate<SLICE>, behind its gathers; the wide body once, behind the gathers of ALL tiles (a pole's 32 tail rows per tile
// need the slice's registers); the row-block bodies walk a per-row table and, once the slice is live, gather in two rounds of
// four.  The chain kernels sit at 256 VGPRs already (tools/kernel_resources.sh): one body templated over the tile count, or
// the row-block table walk folded into db_aggregate, would trade these orders for one that fits none of them.  And a step
// stays written out in a body where the shared statement costs that body registers it does not have: the top layer's head
// backward (shared, db_bwd_chain_kernel spills 7 VGPRs instead of 5), the residual load (db_fwd_chain_kernel spills 41 SGPRs
// instead of 39), and the row-block bodies' (see their section).  profiles/rowblock_resources.txt has the figures.
#include "mfma_tiles.h"
#include "device_facts.h"

namespace {

using namespace geom;

constexpr int DB_THREADS = 256;
constexpr int DB_C = RB_C;           // layer width
constexpr int DB_K = 64;             // aggregated columns (split 3)
constexpr int DB_W = 8;              // neighbour-table width
constexpr int DB_TAIL = GEOM_DEFORM_TAIL; // width of the tail table (entries of a row beyond the neighbour table)
constexpr int DB_RED = 16;           // floats of reduction scratch
#ifdef DB_PROBE_FEW_MFMA // probe build: a sixth of the MFMAs (wrong results)
constexpr int DB_PROBE = TILE_PROBE_FEW_MFMA;
#else
constexpr int DB_PROBE = TILE_PROBE_NONE;
#endif

#ifdef DB_PROBE_STAMPS
// probe build (tools/probe/db_stamps.sh): shader-clock stamps of wave 0 of every workgroup at the phase boundaries
constexpr int DB_STAMP_SLOTS = 16;
__device__ unsigned long long db_stamps[1024 * DB_STAMP_SLOTS];
#define DB_STAMP(i)                                                                                            \
    do {                                                                                                       \
        __builtin_amdgcn_sched_barrier(0);                                                                     \
        if (threadIdx.x == 0) db_stamps[blockIdx.x * DB_STAMP_SLOTS + (i)] = __builtin_amdgcn_s_memtime();     \
        __builtin_amdgcn_sched_barrier(0);                                                                     \
    } while (0)
#else
#define DB_STAMP(i) do { } while (0)
#endif

// ---- the layers of a block as ONE launch (db_fwd_chain_kernel): a vertex's workgroup runs layer after layer and waits, in front
// of a layer's gathers, until the workgroups of its NEIGHBOURS have published the previous layer's support rows -- the only
// cross-tile dependency of a layer (see the top of the file).  done[v * DB_CTR_STRIDE] = layers vertex v has published (a
// 128-byte line each: pollers and publishers of different vertices never share one); zero on entry (the weight-packing launch of
// the step zeroes it).  Every workgroup of the launch must be resident at once (the host checks; otherwise separate launches).
constexpr int DB_CTR_STRIDE = 32;
constexpr int DB_SPIN_LIMIT = 1 << 20; // polls before a wait gives up (seconds): the layer's outputs are then NaN, loudly

// wave-wide wait: lane's `target` vertex (< 0: none) has published `need` layers.  false: gave up.
__device__ __forceinline__ bool db_wait_published(const int *done, int target, int need)
{
    bool ok = target < 0;
    for (int polls = 0;; ++polls) {
        if (!ok) ok = __hip_atomic_load(done + (size_t)target * DB_CTR_STRIDE, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= need;
        if (__all(ok)) return true;
        if (polls > DB_SPIN_LIMIT) return false;
        __builtin_amdgcn_s_sleep(2);
    }
}

// workgroup w -> vertex: contiguous vertex runs per XCD (workgroup w runs on XCD w % 8; a support row is gathered by its ~7
// neighbours, which are mostly near it in the numbering, so a run's rows stay in one L2)
__device__ __forceinline__ int db_vertex(int w, int vpx, int nv)
{
    const int v = (w & 7) * vpx + (w >> 3);
    return ((w >> 3) < vpx && v < nv) ? v : -1;
}

// fixed-order block reduction of two values: wave shuffles, then the four wave partials in order
__device__ __forceinline__ void db_sum2(float &a, float &b, float *red)
{
    for (int off = GEOM_WAVE / 2; off > 0; off >>= 1) {
        a += __shfl_down(a, off, GEOM_WAVE);
        b += __shfl_down(b, off, GEOM_WAVE);
    }
    const int lane = threadIdx.x & (GEOM_WAVE - 1), wave = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) red[2 * wave] = a, red[2 * wave + 1] = b;
    __syncthreads();
    a = ((red[0] + red[2]) + red[4]) + red[6];
    b = ((red[1] + red[3]) + red[5]) + red[7];
}

// The wave's 192 x 48 slice of a weight, from the PACKED copy geom_deform_pack_weights_f32 makes once per step: element
// e = (4 jp + c) * 3 + u of lane (x, g) of wave w is W[k = 48 g + 4 jp + c][48 w + 3 x + u] (the row-block product's slice, mfma_tiles.h),
// stored [wave][e / 4][lane][e % 4] -- every load instruction of a wave reads 1 KB of consecutive bytes (36 b128 loads per
// lane instead of 48 12-byte loads whose 192-byte runs straddle cache lines: 1.67 x fewer L2 bytes -- all 482 workgroups
// read the same 147 KB, the L2 of an XCD is what they queue at).
struct DbSlice {
    f32x4 q[36];
    __device__ __forceinline__ float at(int jp, int c, int u) const { const int e = (4 * jp + c) * 3 + u; return q[e >> 2][e & 3]; }
};
__device__ __forceinline__ void db_load_slice(DbSlice &bw, const float *packed, int wave, int lane)
{
    const __amdgpu_buffer_rsrc_t r_b = rsrc(packed, (int64_t)DB_C * DB_C * 4);
    const unsigned b0 = ((unsigned)(wave * 36) * 64u + (unsigned)lane) * 16u;
#pragma unroll
    for (int i = 0; i < 36; ++i) {
#ifdef DB_PROBE_HOT_SLICE
        const u32x4 t = __builtin_amdgcn_raw_buffer_load_b128(r_b, b0 + (unsigned)(i & 1) * 1024u, 0, 0); // probe: 2 KB per wave (L1 hits)
#else
        const u32x4 t = __builtin_amdgcn_raw_buffer_load_b128(r_b, b0 + (unsigned)i * 1024u, 0, 0);
#endif
        bw.q[i] = (f32x4){__uint_as_float(t.x), __uint_as_float(t.y), __uint_as_float(t.z), __uint_as_float(t.w)};
    }
}

// C tile [16 rows][192] = panel [16][192] . slice, into the staging tile (natural [row][col] layout, pitch RB_LDC)
__device__ __forceinline__ void db_product(const DbSlice &bw, const float *panel, float *stage, int wave, int x, int g)
{
    f32x4 acc[3];
    rowblock_product<DB_PROBE>([&](int jp, int c, int u) { return bw.at(jp, c, u); }, panel + panel_offset(48 * g, x), acc);
    rowblock_to_stage(acc, stage, wave, x, g);
}

// geom_deform_pack_weights_f32: thread = one element of one packed copy (2 * count copies of 36 864 floats)
struct DbPackArgs {
    const float *w[GEOM_DEFORM_MAX_PACK];
    float *fwd, *bwd;
    int count;
    int *zero;      // optional: words to clear (the chain launches' counters), by the workgroups behind the packing ones
    int zero_words, pack_blocks;
};
__global__ __launch_bounds__(256) void db_pack_kernel(DbPackArgs a)
{
    if ((int)blockIdx.x >= a.pack_blocks) {
        const int i = ((int)blockIdx.x - a.pack_blocks) * 256 + (int)threadIdx.x;
        if (i < a.zero_words) a.zero[i] = 0;
        return;
    }
    const int idx = blockIdx.x * 256 + threadIdx.x;
    const int m = idx / (DB_C * DB_C), r = idx - m * (DB_C * DB_C);
    const int layer = m >> 1, dir = m & 1;
    if (layer >= a.count) return;
    const int wave = r / 9216, rem = r - wave * 9216;
    const int i = rem >> 8, lane = (rem & 255) >> 2, t = rem & 3;
    const int e = 4 * i + t, jp = e / 12, c = (e / 3) & 3, u = e % 3;
    const int g = lane >> 4, x = lane & 15;
    const int k = 48 * g + 4 * jp + c, col = 48 * wave + 3 * x + u;
    const float *w = a.w[layer];
    float *out = dir ? a.bwd : a.fwd;
    if (out) out[(size_t)layer * DB_C * DB_C + r] = dir ? w[col * DB_C + k] : w[k * DB_C + col]; // bwd: the slice of W^T
}

// The aggregated float4 of thread (row rl, group j) of vertex v: sum over the vertex's table entries, then its CSR tail, of
// val * src[mesh rl][neighbour][4 j ..] -- the order and arithmetic of zn_aggregate_ell_kernel (a padded slot adds -0.0: no
// value changes, signed zeros included).  `rowbase` = byte offset of mesh rl's first row; rows beyond the batch pass
// mesh_on = false and read zeros.
// The tail (a vertex with more entries than the table: the 33-entry poles of 482.obj) comes as a second, 32-wide table row
// [nv][DB_TAIL] (-1 = padding) that lanes 0..31 of every wave load with ONE vector load in the round trip of the table's
// scalar loads, so a pole's extra neighbour rows are requested TOGETHER with its table rows: the launch ends with its slowest
// workgroup, and a pole that walked its tail eight entries per dependent round trip took 3 x the time of every other vertex
// (26 000 cycles in the gather phase against 8 500: tools/probe/db_stamps.py).
// a vertex's row of the neighbour table + its tail row (round trip 1 of a layer: scalar loads -- the same for every thread of
// the workgroup -- and ONE vector load of the tail row); a chain launch fetches it once for all its layers
// vertex v's row of the neighbour table: scalar loads where v is the same for the whole workgroup (db_table), vector loads per
// row where every row of a tile has its own vertex (the row-block bodies)
__device__ __forceinline__ void db_table_row(const int *ell_col, const float *ell_val, int v, int (&nb)[DB_W], float (&wv)[DB_W])
{
    const int4 ci0 = *reinterpret_cast<const int4 *>(ell_col + (size_t)v * DB_W), ci1 = *reinterpret_cast<const int4 *>(ell_col + (size_t)v * DB_W + 4);
    const float4 wi0 = *reinterpret_cast<const float4 *>(ell_val + (size_t)v * DB_W), wi1 = *reinterpret_cast<const float4 *>(ell_val + (size_t)v * DB_W + 4);
    nb[0] = ci0.x, nb[1] = ci0.y, nb[2] = ci0.z, nb[3] = ci0.w, nb[4] = ci1.x, nb[5] = ci1.y, nb[6] = ci1.z, nb[7] = ci1.w;
    wv[0] = wi0.x, wv[1] = wi0.y, wv[2] = wi0.z, wv[3] = wi0.w, wv[4] = wi1.x, wv[5] = wi1.y, wv[6] = wi1.z, wv[7] = wi1.w;
}
struct DbTable {
    int nb[DB_W];
    float wv[DB_W];
    int tcol;
    float tval;
    bool has_tail;
};
__device__ __forceinline__ DbTable db_table(int v, const int *ell_col, const float *ell_val, const int *tail_col, const float *tail_val,
                                            int lane)
{
    DbTable t;
    t.tcol = -1, t.tval = 0.f;
    if (tail_col) {
        t.tcol = tail_col[(size_t)v * DB_TAIL + (lane & (DB_TAIL - 1))];
        t.tval = tail_val[(size_t)v * DB_TAIL + (lane & (DB_TAIL - 1))];
    }
    db_table_row(ell_col, ell_val, v, t.nb, t.wv);
    t.has_tail = tail_col != nullptr;
    return t;
}

// CHAIN (need > 0): the rows are another workgroup's output of the same launch -- wait until the neighbours have published
// `need` layers (ok = false: the wait gave up), read with agent-scope loads.
template <bool SLICE, bool CHAIN = false>
__device__ __forceinline__ float4 db_aggregate(__amdgpu_buffer_rsrc_t r_src, bool mesh_on, unsigned rowbase, int v, int c0,
                                               const DbTable &tb, float4 *own, DbSlice &bw, const float *packed, int wave, int lane,
                                               const int *done = nullptr, int need = 0, bool *ok = nullptr)
{
    const int (&nb)[DB_W] = tb.nb;
    const float (&wv)[DB_W] = tb.wv;
    const int tcol = tb.tcol;
    const float tval = tb.tval;
    if (CHAIN && need > 0) { // lanes 0..7: the table's neighbours; lanes 8..39: the tail row's
        int target = -1;
#pragma unroll
        for (int n = 0; n < DB_W; ++n) target = lane == n ? nb[n] : target;
        const int from_tail = __shfl(tcol, (lane - DB_W) & (GEOM_WAVE - 1), GEOM_WAVE);
        if (lane >= DB_W && lane < DB_W + DB_TAIL) target = from_tail;
        const bool there = db_wait_published(done, target, need);
        if (!there) *ok = false;
    }
    // round trip 2: the neighbour rows + the thread's own pass-through elements
    float4 sv[DB_W];
#pragma unroll
    for (int n = 0; n < DB_W; ++n) {
        const unsigned off = rowbase + (unsigned)(nb[n] >= 0 ? nb[n] : v) * (DB_C * 4) + 4 * c0;
        sv[n] = ld4<CHAIN>(r_src, mesh_on ? off : OOB);
    }
    const unsigned own_off = rowbase + (unsigned)v * (DB_C * 4) + 4 * c0;
#pragma unroll
    for (int i = 0; i < 2; ++i) own[i] = ld4<CHAIN>(r_src, mesh_on ? own_off + 4 * DB_K * (i + 1) : OOB);
    float4 facc = make_float4(0.f, 0.f, 0.f, 0.f);
    auto table_terms = [&]() {
#pragma unroll
        for (int n = 0; n < DB_W; ++n) {
            const bool in = nb[n] >= 0;
            const float tx = wv[n] * sv[n].x, ty = wv[n] * sv[n].y, tz = wv[n] * sv[n].z, tw = wv[n] * sv[n].w;
            facc.x += in ? tx : -0.0f, facc.y += in ? ty : -0.0f, facc.z += in ? tz : -0.0f, facc.w += in ? tw : -0.0f;
        }
    };
    __builtin_amdgcn_sched_barrier(0);
    const bool has_tail = tb.has_tail && __builtin_amdgcn_readfirstlane(tcol) >= 0; // (uniform: entry 0 of the tail row)
    if (!has_tail) { // every vertex of an icosphere, all but the two poles of 482.obj
        if (SLICE) db_load_slice(bw, packed, wave, lane); // behind the gathers (in-order memory counter: see the callers)
        __builtin_amdgcn_sched_barrier(0);
        table_terms();
        return facc;
    }
    // the tail rows, all in flight at once; the weight slice behind them (its registers hold the tail's rows until then)
    float4 tv[DB_TAIL];
#pragma unroll
    for (int n = 0; n < DB_TAIL; ++n) {
        const int col = __builtin_amdgcn_readlane(tcol, n);
        tv[n] = ld4<CHAIN>(r_src, (mesh_on && col >= 0) ? rowbase + (unsigned)col * (DB_C * 4) + 4 * c0 : OOB);
    }
    table_terms(); // summation order: the table's slots, then the tail, in CSR order
#pragma unroll
    for (int n = 0; n < DB_TAIL; ++n) {
        const bool in = __builtin_amdgcn_readlane(tcol, n) >= 0;
        const float wn = __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(tval), n));
        const float tx = wn * tv[n].x, ty = wn * tv[n].y, tz = wn * tv[n].z, tw = wn * tv[n].w;
        facc.x += in ? tx : -0.0f, facc.y += in ? ty : -0.0f, facc.z += in ? tz : -0.0f, facc.w += in ? tw : -0.0f;
    }
    __builtin_amdgcn_sched_barrier(0);
    if (SLICE) db_load_slice(bw, packed, wave, lane);
    __builtin_amdgcn_sched_barrier(0);
    return facc;
}

__device__ __forceinline__ void db_to_panel(float *panel, int rl, int c0, const float4 (&x)[3])
{
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        *reinterpret_cast<float4 *>(panel + panel_offset(c0 + DB_K * i, rl)) = x[i];
    }
}

// ---- the steps every body of this file shares.  Each is stated ONCE: the wide launches must give the bits of the plain ones
// and the eval launch those of vertex_bn's eval branch, so a body calls these and keeps only its own schedule (the top of the
// file).  Values and fixed-size array references only: the bodies sit at the register ceiling, nothing here may reach scratch.

// byte offset of the thread's float4 i (columns c0 + 64 i ..) of its own row, from that of float4 0 (OOB: no row)
__device__ __forceinline__ unsigned db_own(unsigned own_off, int i) { return own_off == OOB ? OOB : own_off + 4 * DB_K * i; }

template <typename Args> // geom_deform_fwd or geom_deform_infer
__device__ __forceinline__ float4 db_bias4(const Args &a, int c0, int i)
{
    return a.bias ? *reinterpret_cast<const float4 *>(a.bias + c0 + DB_K * i) : make_float4(0.f, 0.f, 0.f, 0.f);
}
__device__ __forceinline__ void db_add_bias(float4 (&z)[3], const float4 (&bias4)[3])
{
#pragma unroll
    for (int i = 0; i < 3; ++i) z[i].x += bias4[i].x, z[i].y += bias4[i].y, z[i].z += bias4[i].z, z[i].w += bias4[i].w;
}

// BatchNorm + ReLU + residual of a thread's 12 values: the operations and order of geom_vertex_bn_fwd_f32 (no folded scale /
// shift).  `on` = false: a row beyond the batch, zeros.
struct DbNorm {
    float mean, invstd, gamma, beta;
};
template <typename Args> // (relu, res and scale are the layer's: geom_deform_fwd or geom_deform_infer)
__device__ __forceinline__ float db_norm_one(const Args &a, const DbNorm &bn, float zz, float r, bool on)
{
    float y = (zz - bn.mean) * bn.invstd * bn.gamma + bn.beta;
    if (a.relu) y = y <= 0.f ? 0.f : y;
    if (a.res) y = (r + y) * a.scale;
    return on ? y : 0.f;
}
template <typename Args>
__device__ __forceinline__ void db_norm_apply(const Args &a, const DbNorm &bn, const float4 (&z)[3], const float4 (&r)[3], bool on, float4 (&xo)[3])
{
#pragma unroll
    for (int i = 0; i < 3; ++i)
        xo[i] = make_float4(db_norm_one(a, bn, z[i].x, r[i].x, on), db_norm_one(a, bn, z[i].y, r[i].y, on),
                            db_norm_one(a, bn, z[i].z, r[i].z, on), db_norm_one(a, bn, z[i].w, r[i].w, on));
}

// batch statistics: a thread's 12 values of one tile row, in this order
__device__ __forceinline__ float db_row_sum(const float4 (&z)[3])
{
    return (((z[0].x + z[0].y) + (z[0].z + z[0].w)) + ((z[1].x + z[1].y) + (z[1].z + z[1].w))) + ((z[2].x + z[2].y) + (z[2].z + z[2].w));
}
__device__ __forceinline__ float db_row_centred_sq(const float4 (&z)[3], float mean)
{
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const float d0 = z[i].x - mean, d1 = z[i].y - mean, d2 = z[i].z - mean, d3 = z[i].w - mean;
        q += (d0 * d0 + d1 * d1) + (d2 * d2 + d3 * d3);
    }
    return q;
}
// ... and what follows the two reductions: q = the vertex's centred sum of squares over its n values.  Returns invstd; thread 0
// writes the saved statistics and moves the running ones (nn.BatchNorm1d: with the unbiased variance).
__device__ __forceinline__ float db_publish_stats(const geom_deform_fwd &a, int v, int n, float mean, float q, float old_mean, float old_var)
{
    const float var = q / n; // biased, as used for normalisation
    const float invstd = 1.f / sqrtf(var + a.eps);
    if (threadIdx.x == 0) {
        a.save_mean[v] = mean, a.save_invstd[v] = invstd;
        if (a.run_mean) a.run_mean[v] = (1.f - a.momentum) * old_mean + a.momentum * mean;
        if (a.run_var) a.run_var[v] = (1.f - a.momentum) * old_var + a.momentum * (n > 1 ? q / (n - 1) : var);
    }
    return invstd;
}

// The coordinate head's product (models.py:219,295: gc15 = 192 -> 3) inside the last hidden layer's launch:
// h[o] = sum_c X[row][c] W_head[c][o]; a row's 192 columns sit in the 16 lanes of its group, every one of which gets the sums
__device__ __forceinline__ void db_head_fwd(const float4 (&xo)[3], const float *w_head, int c0, float (&h)[3])
{
    h[0] = 0.f, h[1] = 0.f, h[2] = 0.f;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const float xv[4] = {xo[i].x, xo[i].y, xo[i].z, xo[i].w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float *wr = w_head + (size_t)(c0 + DB_K * i + e) * 3;
            h[0] += xv[e] * wr[0], h[1] += xv[e] * wr[1], h[2] += xv[e] * wr[2];
        }
    }
#pragma unroll
    for (int m = 8; m > 0; m >>= 1) {
        h[0] += __shfl_xor(h[0], m, GEOM_WAVE), h[1] += __shfl_xor(h[1], m, GEOM_WAVE), h[2] += __shfl_xor(h[2], m, GEOM_WAVE);
    }
}
// ... stored as the raw support s_head[row] = X'[row] . W_head by the first lane of the row's group
__device__ __forceinline__ void db_head_store(const float4 (&xo)[3], const float *w_head, float *s_head, size_t row, bool on, int c0)
{
    float h[3];
    db_head_fwd(xo, w_head, c0, h);
    if (c0 == 0 && on) {
        float *dst = s_head + row * 3;
        dst[0] = h[0], dst[1] = h[1], dst[2] = h[2];
    }
}

// The staging tile leaves in memory order (a row's 768 bytes are contiguous); row_offset(r) = byte offset of staging row r, or
// OOB.  AGENT: rows another workgroup of the same launch gathers.
template <bool AGENT, typename RowOffset>
__device__ __forceinline__ void db_store_tile(const float *stage, __amdgpu_buffer_rsrc_t r_s, RowOffset row_offset)
{
#pragma unroll
    for (int t = 0; t < 3; ++t) {
        const int idx = (int)threadIdx.x + DB_THREADS * t, r = idx / 48, c4 = idx % 48;
        const f32x4 val = *reinterpret_cast<const f32x4 *>(stage + r * RB_LDC + 4 * c4);
        const unsigned row = row_offset(r);
        st4<AGENT>(r_s, row == OOB ? OOB : row + 16u * c4, make_float4(val[0], val[1], val[2], val[3]));
    }
}
// ... or returns to the thread's registers (its row rl, columns c0 + 64 i ..)
__device__ __forceinline__ void db_load_tile(const float *stage, int rl, int c0, float4 (&go)[3])
{
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const f32x4 t = *reinterpret_cast<const f32x4 *>(stage + rl * RB_LDC + c0 + DB_K * i);
        go[i] = make_float4(t[0], t[1], t[2], t[3]);
    }
}

// BatchNorm backward of one element: gg = the upstream gradient (+ the second one, * the residual's scale: returned, the
// residual's gradient), then masked by the ReLU and the batch; xhat and the two sums of the reduction
__device__ __forceinline__ float db_bn_bwd_elem(const geom_deform_bwd &a, float mean, float invstd, float gamma, float beta, bool mesh_on,
                                                float zz, float &gg, float second, float &xhat, float &sum_g, float &sum_gx)
{
    xhat = (zz - mean) * invstd;
    gg += second;
    if (a.has_res) gg *= a.scale;
    const float pass = gg;
    if (a.relu && xhat * gamma + beta <= 0.f) gg = 0.f;
    if (!mesh_on) gg = 0.f;
    sum_g += gg;
    sum_gx += gg * xhat;
    return pass;
}
// ... a float4 of them; the residual's gradient leaves for grad_res at `off`
__device__ __forceinline__ void db_bn_bwd_elems(const geom_deform_bwd &a, float mean, float invstd, float gamma, float beta, bool mesh_on,
                                                const float4 &zv, float4 &go, const float4 &second, float4 &xh, float &sum_g, float &sum_gx,
                                                __amdgpu_buffer_rsrc_t r_gr, unsigned off)
{
    const float4 r = make_float4(db_bn_bwd_elem(a, mean, invstd, gamma, beta, mesh_on, zv.x, go.x, second.x, xh.x, sum_g, sum_gx),
                                 db_bn_bwd_elem(a, mean, invstd, gamma, beta, mesh_on, zv.y, go.y, second.y, xh.y, sum_g, sum_gx),
                                 db_bn_bwd_elem(a, mean, invstd, gamma, beta, mesh_on, zv.z, go.z, second.z, xh.z, sum_g, sum_gx),
                                 db_bn_bwd_elem(a, mean, invstd, gamma, beta, mesh_on, zv.w, go.w, second.w, xh.w, sum_g, sum_gx));
    if (a.has_res && a.grad_res) st4(r_gr, off, r);
}
// after the reduction: the BatchNorm parameter gradients of vertex v
__device__ __forceinline__ void db_publish_bn_grads(const geom_deform_bwd &a, int v, float sum_g, float sum_gx)
{
    if (threadIdx.x == 0) {
        if (a.grad_bn_b) a.grad_bn_b[v] = sum_g;
        if (a.grad_bn_w) a.grad_bn_w[v] = sum_gx;
    }
}
__device__ __forceinline__ float db_bn_bwd_dz(float kk, float g, float xhat, float mg, float mgx) { return kk * (g - mg - xhat * mgx); }
__device__ __forceinline__ float4 db_bn_bwd_dz4(float kk, const float4 &g, const float4 &xh, float mg, float mgx, bool mesh_on)
{
    float4 dz = make_float4(db_bn_bwd_dz(kk, g.x, xh.x, mg, mgx), db_bn_bwd_dz(kk, g.y, xh.y, mg, mgx), db_bn_bwd_dz(kk, g.z, xh.z, mg, mgx),
                            db_bn_bwd_dz(kk, g.w, xh.w, mg, mgx));
    if (!mesh_on) dz = make_float4(0.f, 0.f, 0.f, 0.f);
    return dz;
}

// Bias gradient of a layer: the vertex's column sums of `src` (a thread's dZ, summed over its tiles) over its meshes, in mesh
// order -- lanes 16 apart hold the wave's four rows, the four waves' sums through the staging tile; the host adds the vertices up
__device__ __forceinline__ void db_colsum(const float4 (&src)[3], float *stage, float *colsum, int v, int c0)
{
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    __syncthreads(); // (the staging tile may still be read above)
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        float4 t = src[i];
#pragma unroll
        for (int k = 1; k < 4; ++k) {
            const int from = (lane & 15) + 16 * k;
            t.x += __shfl(src[i].x, from), t.y += __shfl(src[i].y, from), t.z += __shfl(src[i].z, from), t.w += __shfl(src[i].w, from);
        }
        if ((lane >> 4) == 0) *reinterpret_cast<float4 *>(stage + wave * DB_C + c0 + DB_K * i) = t;
    }
    __syncthreads();
    if (tid < DB_C) colsum[(size_t)v * DB_C + tid] = ((stage[tid] + stage[DB_C + tid]) + stage[2 * DB_C + tid]) + stage[3 * DB_C + tid];
}

// The coordinate head's backward (gc15, 192 -> 3) inside the first backward launch: dS_head . W_head^T of column `col` joins g ...
__device__ __forceinline__ float db_head_bwd_input(const float (&dsh)[3], const float *w_head, int col)
{
    const float *wr = w_head + (size_t)col * 3;
    return (dsh[0] * wr[0] + dsh[1] * wr[1]) + dsh[2] * wr[2];
}
// ... and the vertex's partial of its weight gradient X^T . dS_head goes out with the column sums.  p = the thread's product
// (summed over its tiles) for (col, o): the rows of a wave (lanes 16 apart, in mesh order) into wsum [4 waves][192 * 3],
__device__ __forceinline__ void db_head_bwd_weight_rows(float p, float *wsum, int col, int o)
{
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    float acc = p;
#pragma unroll
    for (int k = 1; k < 4; ++k) acc += __shfl(p, (lane & 15) + 16 * k, GEOM_WAVE);
    if ((lane >> 4) == 0) wsum[wave * (DB_C * 3) + col * 3 + o] = acc;
}
// then the four waves in order
__device__ __forceinline__ void db_head_bwd_weight_reduce(const float *wsum, float *dw_head, int v)
{
    __syncthreads();
    for (int t = threadIdx.x; t < DB_C * 3; t += DB_THREADS)
        dw_head[(size_t)v * (DB_C * 3) + t] = ((wsum[t] + wsum[DB_C * 3 + t]) + wsum[2 * DB_C * 3 + t]) + wsum[3 * DB_C * 3 + t];
    __syncthreads();
}

// G = [A^T . dZ[:, :64] | dZ[:, 64:]] of the thread's row (an aggregation backward: db_aggregate on the transposed tables),
// kept in gs and stored at its own place of r_dst.  CHAIN and the wait gave up: NaN, loudly.
template <bool SLICE, bool CHAIN>
__device__ __forceinline__ void db_aggregate_and_store_own_row(__amdgpu_buffer_rsrc_t r_src, __amdgpu_buffer_rsrc_t r_dst, bool mesh_on,
                                                               unsigned rowbase, int v, int c0, const DbTable &tb, float4 (&gs)[3], DbSlice &bw,
                                                               const float *packed, int wave, int lane, const int *done = nullptr,
                                                               int need = 0)
{
    bool arrived = true;
    gs[0] = db_aggregate<SLICE, CHAIN>(r_src, mesh_on, rowbase, v, c0, tb, &gs[1], bw, packed, wave, lane, done, need, &arrived);
    if (CHAIN && !arrived) gs[0].x = __builtin_nanf("");
    const unsigned own_off = mesh_on ? rowbase + (unsigned)v * (DB_C * 4) + 4 * c0 : OOB;
#pragma unroll
    for (int i = 0; i < 3; ++i) st4(r_dst, db_own(own_off, i), gs[i]);
}

// One layer of vertex v.  CHAIN: layer `layer` (0-based) of a chain launch -- layer > 0 reads the previous layer's support
// rows from the neighbours' workgroups (wait + agent-scope loads), a layer with a product publishes its rows.
template <bool PRODUCT, bool CHAIN>
__device__ __forceinline__ void db_fwd_body(const geom_deform_fwd &a, const int v, float *lds, int *done, const int layer,
                                            const DbTable *table)
{
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int x = lane & 15, g = lane >> 4; // matrix-core coordinates
    const int rl = tid >> 4, j = tid & 15;  // batch row (mesh) and float4 group of the gather / BatchNorm thread
    const int c0 = 4 * j;
    DB_STAMP(0);
    const bool mesh_on = rl < a.b;
    const int64_t op_bytes = (int64_t)a.b * a.nv * DB_C * 4;
    const __amdgpu_buffer_rsrc_t r_src = rsrc(a.s_in, op_bytes);
    const unsigned rowbase = (unsigned)rl * (unsigned)a.nv * (DB_C * 4);
    const unsigned own_off = mesh_on ? rowbase + (unsigned)v * (DB_C * 4) + 4 * c0 : OOB;
    // the vertex's BatchNorm parameters, the bias and the residual travel with the gathers
    const float gamma = a.bn_w ? a.bn_w[v] : 1.f, beta = a.bn_b ? a.bn_b[v] : 0.f;
    const bool updates = a.training && tid == 0;
    const float old_mean = (updates && a.run_mean) ? a.run_mean[v] : 0.f, old_var = (updates && a.run_var) ? a.run_var[v] : 0.f;
    float4 bias4[3], rv[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) bias4[i] = db_bias4(a, c0, i), rv[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (a.res) {
        const __amdgpu_buffer_rsrc_t r_res = rsrc(a.res, ((int64_t)a.b * a.nv - 1) * a.res_ld * 4 + DB_C * 4);
        const unsigned roff = ((unsigned)rl * (unsigned)a.nv + (unsigned)v) * (unsigned)a.res_ld * 4u + 4 * c0;
#pragma unroll
        for (int i = 0; i < 3; ++i) rv[i] = ld4(r_res, mesh_on ? roff + 4 * DB_K * i : OOB);
    }
    // The weight slice is requested BEHIND the gathers: the vector-memory counter retires in order, so a wave that asked for
    // its 36 KB of weights first would wait for them in front of every gather (the table entries come by scalar loads, which
    // have a counter of their own); in this order the statistics run while the slice is still on its way.
    DbSlice bw;
    float4 z[3];
    bool arrived = true; // (a chain launch: the neighbours' rows were published in time)
    if (CHAIN) {
        z[0] = db_aggregate<PRODUCT, true>(r_src, mesh_on, rowbase, v, c0, *table, &z[1], bw, a.w_next, wave, lane, done, layer, &arrived);
    } else {
        const DbTable tb = db_table(v, a.ell_col, a.ell_val, a.tail_col, a.tail_val, lane);
        z[0] = db_aggregate<PRODUCT, false>(r_src, mesh_on, rowbase, v, c0, tb, &z[1], bw, a.w_next, wave, lane);
    }
    if (CHAIN && !arrived) z[0].x = __builtin_nanf(""); // poisons the vertex's statistics: every output of the layer is NaN
    db_add_bias(z, bias4);

    DB_STAMP(1); // gathers arrived (z holds the aggregated row)
    // ---- BatchNorm1d(verts): one statistic per vertex over its b * 192 values (two-pass: mean, then the centred second moment)
    float *red = lds + RB_PANEL + RB_CST;
    const int n = a.b * DB_C;
    DbNorm bn;
    if (a.training) {
        float s = 0.f, dummy = 0.f;
        if (mesh_on) s = db_row_sum(z);
        db_sum2(s, dummy, red);
        bn.mean = s / n;
        float q = 0.f;
        if (mesh_on) q = db_row_centred_sq(z, bn.mean);
        dummy = 0.f;
        db_sum2(q, dummy, red);
        bn.invstd = db_publish_stats(a, v, n, bn.mean, q, old_mean, old_var);
    } else {
        bn.mean = a.run_mean[v];
        bn.invstd = 1.f / sqrtf(a.run_var[v] + a.eps);
    }
    bn.gamma = gamma, bn.beta = beta;
    DB_STAMP(2); // statistics done
    float4 xo[3];
    db_norm_apply(a, bn, z, rv, mesh_on, xo);
    const __amdgpu_buffer_rsrc_t r_z = rsrc(a.z_out, op_bytes), r_x = rsrc(a.x_out, op_bytes);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        if (a.z_out) st4(r_z, db_own(own_off, i), z[i]);
        st4(r_x, db_own(own_off, i), xo[i]);
    }
    if (!PRODUCT) {
        // ---- the coordinate head's product inside the last hidden layer's launch
        if (a.w_head && a.s_head) db_head_store(xo, a.w_head, a.s_head, (size_t)rl * a.nv + v, mesh_on, c0);
        return;
    }

    // ---- the next layer's product on the tile
    db_to_panel(lds, rl, c0, xo);
    DB_STAMP(3); // outputs requested, panel written
    __syncthreads();
    DB_STAMP(4);
    float *stage = lds + RB_PANEL;
#ifdef DB_PROBE_STAMPS
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // probe: separate the wait for the weight slice from the MFMAs
    DB_STAMP(5);
#endif
    db_product(bw, lds, stage, wave, x, g);
    DB_STAMP(6); // MFMAs issued + staged
    __syncthreads();
    DB_STAMP(7);
    const __amdgpu_buffer_rsrc_t r_s = rsrc(a.s_out, op_bytes);
    db_store_tile<CHAIN>(stage, r_s, [&](int r) { return r < a.b ? ((unsigned)r * (unsigned)a.nv + (unsigned)v) * (DB_C * 4) : OOB; });
    DB_STAMP(8);
    if (CHAIN) { // publish: every wave's stores are acknowledged (written through), then the vertex's count moves
        __builtin_amdgcn_s_waitcnt(0);
        __syncthreads();
        if (tid == 0) __hip_atomic_store(done + (size_t)v * DB_CTR_STRIDE, layer + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

template <bool PRODUCT>
__global__ __launch_bounds__(DB_THREADS, 2) void db_fwd_kernel(geom_deform_fwd a)
{
    __shared__ __attribute__((aligned(16))) float lds[RB_PANEL + RB_CST + DB_RED];
    const int v = db_vertex(blockIdx.x, a.vpx, a.nv);
    if (v < 0) return;
    db_fwd_body<PRODUCT, false>(a, v, lds, nullptr, 0, nullptr);
}

struct DbFwdChain {
    geom_deform_fwd layer[GEOM_DEFORM_CHAIN_MAX];
    int count;
    int *done;
};

__global__ __launch_bounds__(DB_THREADS, 2) void db_fwd_chain_kernel(DbFwdChain c)
{
    __shared__ __attribute__((aligned(16))) float lds[RB_PANEL + RB_CST + DB_RED];
    const int v = db_vertex(blockIdx.x, c.layer[0].vpx, c.layer[0].nv);
    if (v < 0) return;
    const DbTable tb = db_table(v, c.layer[0].ell_col, c.layer[0].ell_val, c.layer[0].tail_col, c.layer[0].tail_val, threadIdx.x & 63);
    for (int l = 0; l < c.count; ++l) {
        if (c.layer[l].w_next) db_fwd_body<true, true>(c.layer[l], v, lds, c.done, l, &tb);
        else db_fwd_body<false, true>(c.layer[l], v, lds, c.done, l, &tb);
        __syncthreads(); // (the layer's LDS is free again)
    }
}

// One backward layer of vertex v.  CHAIN: step `step` of a chain launch (0 = the top layer) -- a step > 0 gathers the dZ rows
// the neighbours' workgroups wrote in the step before (wait + agent-scope loads); every step publishes its dZ rows.
template <bool PRODUCT, bool CHAIN>
__device__ __forceinline__ void db_bwd_body(const geom_deform_bwd &a, const int v, float *lds, int *done, const int step,
                                            const DbTable *table)
{
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int x = lane & 15, g = lane >> 4;
    const int rl = tid >> 4, j = tid & 15;
    const int c0 = 4 * j;
    DB_STAMP(0);
    const bool mesh_on = rl < a.b;
    const int64_t op_bytes = (int64_t)a.b * a.nv * DB_C * 4;
    const unsigned rowbase = (unsigned)rl * (unsigned)a.nv * (DB_C * 4);
    const unsigned own_off = mesh_on ? rowbase + (unsigned)v * (DB_C * 4) + 4 * c0 : OOB;
    // everything this layer's BatchNorm backward reads is requested with the gathers
    // g / g2 may be column slices of wider row-major buffers (row pitch g_ld / g2_ld floats; dword-aligned 16-byte buffer loads):
    // the next block's input gradient is read in place instead of through a slicing copy
    const int g_ld = a.g_ld ? a.g_ld : DB_C, g2_ld = a.g2_ld ? a.g2_ld : DB_C;
    const __amdgpu_buffer_rsrc_t r_z = rsrc(a.z, op_bytes);
    const __amdgpu_buffer_rsrc_t r_g2 = rsrc(a.g2, ((int64_t)a.b * a.nv - 1) * g2_ld * 4 + DB_C * 4);
    const __amdgpu_buffer_rsrc_t r_g = rsrc(a.g, ((int64_t)a.b * a.nv - 1) * g_ld * 4 + DB_C * 4);
    const unsigned g_off = mesh_on ? (((unsigned)rl * (unsigned)a.nv + (unsigned)v) * (unsigned)g_ld + (unsigned)c0) * 4u : OOB;
    const unsigned g2_off = mesh_on ? (((unsigned)rl * (unsigned)a.nv + (unsigned)v) * (unsigned)g2_ld + (unsigned)c0) * 4u : OOB;
    const float mean = a.save_mean[v], invstd = a.save_invstd[v];
    const float gamma = a.bn_w ? a.bn_w[v] : 1.f, beta = a.bn_b ? a.bn_b[v] : 0.f;
    float4 zv[3], g2v[3], go[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        zv[i] = ld4(r_z, db_own(own_off, i));
        g2v[i] = a.g2 ? ld4(r_g2, db_own(g2_off, i)) : make_float4(0.f, 0.f, 0.f, 0.f);
        if (!PRODUCT) go[i] = a.g ? ld4(r_g, db_own(g_off, i)) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    if (!PRODUCT && a.ds_head) {
        // ---- the coordinate head inside the first backward launch (db_head_bwd_*)
        float dsh[3] = {0.f, 0.f, 0.f};
        if (mesh_on) {
            const float *src = a.ds_head + ((size_t)rl * a.nv + v) * 3;
            dsh[0] = src[0], dsh[1] = src[1], dsh[2] = src[2];
        }
        const __amdgpu_buffer_rsrc_t r_xt = rsrc(a.x_top, op_bytes);
        float *wsum = lds + RB_PANEL; // [4 waves][192 * 3]
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const float4 xt = a.dw_head ? ld4(r_xt, db_own(own_off, i)) : make_float4(0.f, 0.f, 0.f, 0.f);
            const float xv[4] = {xt.x, xt.y, xt.z, xt.w};
            float add[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int col = c0 + DB_K * i + e;
                add[e] = db_head_bwd_input(dsh, a.w_head, col);
                if (a.dw_head) {
#pragma unroll
                    for (int o = 0; o < 3; ++o) db_head_bwd_weight_rows(xv[e] * dsh[o], wsum, col, o);
                }
            }
            go[i].x += add[0], go[i].y += add[1], go[i].z += add[2], go[i].w += add[3];
        }
        if (a.dw_head) db_head_bwd_weight_reduce(wsum, a.dw_head, v);
    }
    float *stage = lds + RB_PANEL;
    if (PRODUCT) {
        // ---- aggregation backward of the layer above: G = [A^T . dZ_up[:, :64] | dZ_up[:, 64:]]
        const __amdgpu_buffer_rsrc_t r_src = rsrc(a.dz_up, op_bytes), r_ds = rsrc(a.ds_up, op_bytes);
        float4 gs[3]; // (stored: the layer above's weight gradient reads it, X^T . G)
        DbSlice bw;
        if (CHAIN) {
            db_aggregate_and_store_own_row<true, true>(r_src, r_ds, mesh_on, rowbase, v, c0, *table, gs, bw, a.wt_up, wave, lane, done, step);
        } else {
            const DbTable tb = db_table(v, a.ell_col_t, a.ell_val_t, a.tail_col_t, a.tail_val_t, lane);
            db_aggregate_and_store_own_row<true, false>(r_src, r_ds, mesh_on, rowbase, v, c0, tb, gs, bw, a.wt_up, wave, lane);
        }
        db_to_panel(lds, rl, c0, gs);                           // (rows beyond the batch read zeros: zero rows of the tile)
        DB_STAMP(1); // gathers arrived, G stored + in the panel
        __syncthreads();
        DB_STAMP(2);
#ifdef DB_PROBE_STAMPS
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        DB_STAMP(3);
#endif
        db_product(bw, lds, stage, wave, x, g);                 // dX = G . W_up^T
        DB_STAMP(4);
        __syncthreads();
        DB_STAMP(5);
        db_load_tile(stage, rl, c0, go);
    }
    // ---- this layer: residual scale, ReLU mask, BatchNorm backward
    float sum_g = 0.f, sum_gx = 0.f;
    float4 xh[3];
    const __amdgpu_buffer_rsrc_t r_gr = rsrc(a.grad_res, op_bytes), r_dz = rsrc(a.dz, op_bytes);
#pragma unroll
    for (int i = 0; i < 3; ++i)
        db_bn_bwd_elems(a, mean, invstd, gamma, beta, mesh_on, zv[i], go[i], g2v[i], xh[i], sum_g, sum_gx, r_gr, db_own(own_off, i));
    float *red = lds + RB_PANEL + RB_CST;
    DB_STAMP(6);
    db_sum2(sum_g, sum_gx, red);
    DB_STAMP(7);
    db_publish_bn_grads(a, v, sum_g, sum_gx);
    const int n = a.b * DB_C;
    const float kk = gamma * invstd, mg = sum_g / n, mgx = sum_gx / n;
    float4 dz[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        dz[i] = db_bn_bwd_dz4(kk, go[i], xh[i], mg, mgx, mesh_on);
        st4<CHAIN>(r_dz, db_own(own_off, i), dz[i]);
    }
    if (a.colsum) db_colsum(dz, stage, a.colsum, v, c0); // the bias gradient of this layer
    DB_STAMP(8);
    if (CHAIN) { // publish the vertex's dZ rows (every wave's stores acknowledged first)
        __builtin_amdgcn_s_waitcnt(0);
        __syncthreads();
        if (tid == 0) __hip_atomic_store(done + (size_t)v * DB_CTR_STRIDE, step + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

template <bool PRODUCT>
__global__ __launch_bounds__(DB_THREADS, 2) void db_bwd_kernel(geom_deform_bwd a)
{
    __shared__ __attribute__((aligned(16))) float lds[RB_PANEL + RB_CST + DB_RED];
    const int v = db_vertex(blockIdx.x, a.vpx, a.nv);
    if (v < 0) return;
    db_bwd_body<PRODUCT, false>(a, v, lds, nullptr, 0, nullptr);
}

struct DbBwdChain {
    geom_deform_bwd layer[GEOM_DEFORM_CHAIN_MAX]; // in execution order: the top layer first
    int count;
    int *done;
    float *ds_first; // optional: [A^T . dZ[:, :64] | dZ[:, 64:]] of the LAST step's dZ (the first layer's support gradient)
};

__global__ __launch_bounds__(DB_THREADS, 2) void db_bwd_chain_kernel(DbBwdChain c)
{
    __shared__ __attribute__((aligned(16))) float lds[RB_PANEL + RB_CST + DB_RED];
    const int v = db_vertex(blockIdx.x, c.layer[0].vpx, c.layer[0].nv);
    if (v < 0) return;
    const geom_deform_bwd &t = c.layer[c.count > 1 ? 1 : 0]; // (the top layer may come without tables)
    const DbTable tb = db_table(v, t.ell_col_t, t.ell_val_t, t.tail_col_t, t.tail_val_t, threadIdx.x & 63);
    for (int l = 0; l < c.count; ++l) {
        if (c.layer[l].dz_up) db_bwd_body<true, true>(c.layer[l], v, lds, c.done, l, &tb);
        else db_bwd_body<false, true>(c.layer[l], v, lds, c.done, l, &tb);
        __syncthreads();
    }
    if (c.ds_first) {
        // one more hand-off instead of one more launch: the aggregation backward of the chain's first layer (no activation, no
        // product behind it: the first layer's products stay with the caller) -- the bits of geom_zn_gcn_aggregate_ell_bwd_f32
        const geom_deform_bwd &a = c.layer[c.count - 1];
        const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
        const int rl = tid >> 4, c0 = 4 * (tid & 15);
        const bool mesh_on = rl < a.b;
        const int64_t op_bytes = (int64_t)a.b * a.nv * DB_C * 4;
        const unsigned rowbase = (unsigned)rl * (unsigned)a.nv * (DB_C * 4);
        const __amdgpu_buffer_rsrc_t r_src = rsrc(a.dz, op_bytes), r_ds = rsrc(c.ds_first, op_bytes);
        float4 gs[3];
        DbSlice none;
        db_aggregate_and_store_own_row<false, true>(r_src, r_ds, mesh_on, rowbase, v, c0, tb, gs, none, nullptr, wave, lane, c.done, c.count);
    }
}

// ---- the row-block launches, one per hidden layer and direction: the eval-mode forward (geom_deform_infer_fwd_f32:
// di_row_block, di_fwd_kernel) and the BatchNorm-free block of the old driver on split meshes (geom_deform_plain_{fwd,bwd}_f32:
// dp_fwd_row_block, dp_bwd_row_block; reference models.py:138-201 on old_GEOMetrics/layers.py:106-149)
//
//   Z   = [A . S[:, :64] | S[:, 64:]] + bias          zn_gcn.hip's order and arithmetic (table slots, then the row's tail, in CSR order)
//   X'  = ReLU((Z - rm_v) * (1 / sqrtf(rv_v + eps)) * gamma_v + beta_v) (+ residual, * scale)   eval: vertex_bn.hip's eval branch
//   X'  = relu?(Z) (+ residual, * scale)               plain: NO BatchNorm step (absent, not an identity map: (z - 0) * 1 * 1 + 0
//                                                      would turn -0.0 into +0.0)
//   S'  = X' . W_next                                  exact fp32 on v_mfma_f32_16x16x4_f32 (db_product)
//
// Tiling: in eval mode BatchNorm1d(verts) is a fixed per-vertex affine map and the plain block has none -- no reduction over the
// batch is left -- so the rows are independent apart from the gather, and the tile is 16 CONSECUTIVE rows of the flattened
// [b * nv] row space (a row-block; it may span two meshes: every row gathers inside its own mesh).  At the driver's validation
// batch of 1, and on the ONE unbatched mesh of the old driver, that fills the MFMA rows the training tiling (one vertex = one
// tile, its batch rows = the tile's rows) leaves 15/16 empty, and any batch works.  The table, the BatchNorm parameters and the
// statistics are per ROW here (vector loads; the training kernel has one vertex per workgroup and reads them with scalar loads).
// A row's tail is walked four entries per round trip by the row's own 16 lanes, up to the row's own end (the rows of a wave have
// different lengths; the wave's weight slice is live across the walk: there are no registers for more).  The eval launch reads
// the training launches' second table, [nv][DB_TAIL] with -1 padding (the 33-entry poles of 482.obj); the plain launches a CSR
// overflow list of ANY length -- the old driver's vertex count grows with every face split and its rows get long (a pole of 65
// entries after one split of 482.obj).
//
// Work per workgroup: a workgroup keeps the wave's 192 x 48 weight slice in registers (36 KB per wave, 147 KB per workgroup)
// and runs q or q + 1 consecutive row-blocks (db_deal_row_blocks) over at most DI_WGS = 512 workgroups -- two per CU of an
// MI355X, the residency of __launch_bounds__(256, 2).  Batch 1 (31 row-blocks) and batch 16 (482) get one row-block per
// workgroup: the launch is one latency chain (table -> gathers -> product), and more workgroups are more chains in flight.
// Above 512 row-blocks a workgroup takes two or more in turn instead of a new workgroup re-reading the 147 KB slice from L2:
// at batch 40 (1 205 row-blocks) 512 slices are read instead of 1 205.  Logical workgroup order follows db_vertex: contiguous
// row-block runs per XCD, so the neighbour rows a run gathers stay in one L2.
// No workgroup waits for another: a launch depends only on the one before it in stream order.
//
// The plain block's backward launch: aggregation backward of the layer above + its input-gradient product + this layer's mask,
// with the bias-gradient (and head-weight) partials per ROW-BLOCK -- whichever workgroup runs a row-block writes the same partial
// row.
//
// The eval body and the plain forward body run the same steps and stay two texts: their tails are different data, one four-entry
// step for both walkers adds 16 loads to each eval kernel, and dp_fwd_kernel<false> -- at 96 VGPRs, the last count with 5 waves
// per SIMD -- needs 98 with the row-block geometry as a value struct, with a shared residual load or with db_head_store
// (profiles/rowblock_resources.txt has each variant's figures).
constexpr int DI_WGS = 512;

// The aggregated float4 of a thread's row v in the plain launches: table slots, then the CSR overflow entries [over_ptr[v],
// over_ptr[v + 1]), in CSR order (zn_gcn.hip's order and arithmetic).  ROUND table rows are in flight at once; LOAD_SLICE: the
// wave's weight slice is requested behind the first round.
template <bool LOAD_SLICE, int ROUND>
__device__ __forceinline__ float4 db_row_aggregate(__amdgpu_buffer_rsrc_t r_src, bool on, unsigned rowbase, int v, int c0, const int *ell_col,
                                                   const float *ell_val, const int *over_ptr, const int *over_col, const float *over_val,
                                                   DbSlice &bw, const float *packed, int wave, int lane)
{
    int nb[DB_W];
    float wv[DB_W];
    db_table_row(ell_col, ell_val, v, nb, wv);
    int e = 0, end = 0; // the row's overflow entries [e, end)
    if (over_ptr && on) e = over_ptr[v], end = over_ptr[v + 1];
    float4 facc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int n0 = 0; n0 < DB_W; n0 += ROUND) {
        float4 sv[ROUND];
#pragma unroll
        for (int n = 0; n < ROUND; ++n)
            sv[n] = ld4(r_src, on ? rowbase + (unsigned)(nb[n0 + n] >= 0 ? nb[n0 + n] : v) * (DB_C * 4) + 4 * c0 : OOB);
        if (LOAD_SLICE && n0 == 0) db_load_slice(bw, packed, wave, lane);
#pragma unroll
        for (int n = 0; n < ROUND; ++n) {
            if (nb[n0 + n] >= 0) { // ELL order == CSR order of the row
                facc.x += wv[n0 + n] * sv[n].x, facc.y += wv[n0 + n] * sv[n].y, facc.z += wv[n0 + n] * sv[n].z, facc.w += wv[n0 + n] * sv[n].w;
            }
        }
    }
    for (; e < end; e += 4) { // (a group of 16 lanes leaves at its own row's end)
        int tc[4];
        float tw[4];
        float4 tv[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int at = e + t < end ? e + t : end - 1;
            tc[t] = over_col[at], tw[t] = over_val[at];
        }
#pragma unroll
        for (int t = 0; t < 4; ++t) tv[t] = ld4(r_src, e + t < end ? rowbase + (unsigned)tc[t] * (DB_C * 4) + 4 * c0 : OOB);
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            if (e + t < end) {
                facc.x += tw[t] * tv[t].x, facc.y += tw[t] * tv[t].y, facc.z += tw[t] * tv[t].z, facc.w += tw[t] * tv[t].w;
            }
        }
    }
    return facc;
}

// relu?(Z) (+ residual, * scale) of one element; `on` = false: a row beyond the last, zero
__device__ __forceinline__ float dp_act_one(const geom_deform_plain_fwd &a, float zz, float r, bool on)
{
    float y = zz;
    if (a.relu) y = y <= 0.f ? 0.f : y;
    if (a.res) y = (r + y) * a.scale;
    return on ? y : 0.f;
}

template <bool PRODUCT, bool LOAD_SLICE>
__device__ __forceinline__ void dp_fwd_row_block(const geom_deform_plain_fwd &a, const int rb, float *lds, DbSlice &bw)
{
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int x = lane & 15, g = lane >> 4; // matrix-core coordinates
    const int rl = tid >> 4, j = tid & 15;  // row of the block and float4 group of the gather thread
    const int c0 = 4 * j;
    const int rows = a.b * a.nv;
    const int r = rb * 16 + rl;
    const bool on = r < rows;
    const int mesh = on ? r / a.nv : 0, v = on ? r - mesh * a.nv : 0;
    const int64_t op_bytes = (int64_t)rows * DB_C * 4;
    const __amdgpu_buffer_rsrc_t r_src = rsrc(a.s_in, op_bytes);
    const unsigned rowbase = (unsigned)mesh * (unsigned)a.nv * (DB_C * 4);
    const unsigned own_off = on ? (unsigned)r * (DB_C * 4) + 4 * c0 : OOB;
    // round trip 1: the bias and the residual; the row's table behind them, inside db_row_aggregate
    float4 bias4[3], rv[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) bias4[i] = db_bias4(a, c0, i), rv[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (a.res) {
        const __amdgpu_buffer_rsrc_t r_res = rsrc(a.res, ((int64_t)rows - 1) * a.res_ld * 4 + DB_C * 4);
        const unsigned roff = (unsigned)r * (unsigned)a.res_ld * 4u + 4 * c0;
#pragma unroll
        for (int i = 0; i < 3; ++i) rv[i] = ld4(r_res, on ? roff + 4 * DB_K * i : OOB);
    }
    // round trip 2 (the row's table in front of it): the neighbour rows + the thread's own pass-through elements, the weight
    // slice behind them.  A later row-block of the workgroup holds the slice already: its table rows go in two rounds of four
    // (no registers for eight rows in flight beside the slice)
    constexpr int ROUND = LOAD_SLICE || !PRODUCT ? DB_W : DB_W / 2;
    float4 z[3];
#pragma unroll
    for (int i = 1; i < 3; ++i) z[i] = ld4(r_src, db_own(own_off, i));
    z[0] = db_row_aggregate<LOAD_SLICE, ROUND>(r_src, on, rowbase, v, c0, a.ell_col, a.ell_val, a.over_ptr, a.over_col, a.over_val, bw,
                                               a.w_next, wave, lane);
    db_add_bias(z, bias4);
    float4 xo[3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
        xo[i] = make_float4(dp_act_one(a, z[i].x, rv[i].x, on), dp_act_one(a, z[i].y, rv[i].y, on), dp_act_one(a, z[i].z, rv[i].z, on),
                            dp_act_one(a, z[i].w, rv[i].w, on));
    if (a.z_out) {
        const __amdgpu_buffer_rsrc_t r_z = rsrc(a.z_out, op_bytes);
#pragma unroll
        for (int i = 0; i < 3; ++i) st4(r_z, db_own(own_off, i), z[i]);
    }
    if (a.x_out) {
        const __amdgpu_buffer_rsrc_t r_x = rsrc(a.x_out, op_bytes);
#pragma unroll
        for (int i = 0; i < 3; ++i) st4(r_x, db_own(own_off, i), xo[i]);
    }
    if (!PRODUCT) {
        if (a.w_head) { // db_head_store, written out: through it dp_fwd_kernel<false> takes 98 VGPRs, a wave per SIMD fewer
            float h[3];
            db_head_fwd(xo, a.w_head, c0, h);
            if (j == 0 && on) {
                float *dst = a.s_head + (size_t)r * 3;
                dst[0] = h[0], dst[1] = h[1], dst[2] = h[2];
            }
        }
        return;
    }
    db_to_panel(lds, rl, c0, xo); // (rows beyond the last are zero rows of the panel)
    __syncthreads();
    float *stage = lds + RB_PANEL;
    db_product(bw, lds, stage, wave, x, g);
    __syncthreads();
    const __amdgpu_buffer_rsrc_t r_s = rsrc(a.s_out, op_bytes);
    db_store_tile<false>(stage, r_s, [&](int rr) { // (16 consecutive rows = 12 KB contiguous)
        const int row = rb * 16 + rr;
        return row < rows ? (unsigned)row * (DB_C * 4) : OOB;
    });
    // (the next row-block writes the panel, which nobody reads any more; the staging tile only after its first barrier)
}

// The eval launch's row-block: the same steps on its own schedule (see the section's last paragraph)
template <bool PRODUCT, bool LOAD_SLICE>
__device__ __forceinline__ void di_row_block(const geom_deform_infer &a, const int rb, float *lds, DbSlice &bw)
{
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int x = lane & 15, g = lane >> 4; // matrix-core coordinates
    const int rl = tid >> 4, j = tid & 15;  // row of the block and float4 group of the gather / BatchNorm thread
    const int c0 = 4 * j;
    const int rows = a.b * a.nv;
    const int r = rb * 16 + rl;
    const bool on = r < rows;
    const int mesh = on ? r / a.nv : 0, v = on ? r - mesh * a.nv : 0;
    const int64_t op_bytes = (int64_t)rows * DB_C * 4;
    const __amdgpu_buffer_rsrc_t r_src = rsrc(a.s_in, op_bytes);
    const unsigned rowbase = (unsigned)mesh * (unsigned)a.nv * (DB_C * 4);
    const unsigned own_off = on ? (unsigned)r * (DB_C * 4) + 4 * c0 : OOB;
    // round trip 1: the row's table, the first entry of its tail row, the vertex's BatchNorm parameters and running
    // statistics, the bias and the residual
    int nb[DB_W];
    float wv[DB_W];
    db_table_row(a.ell_col, a.ell_val, v, nb, wv);
    const int tail0 = a.tail_col ? a.tail_col[(size_t)v * DB_TAIL] : -1;
    const float gamma = a.bn_w ? a.bn_w[v] : 1.f, beta = a.bn_b ? a.bn_b[v] : 0.f;
    const float mean = a.run_mean[v], invstd = 1.f / sqrtf(a.run_var[v] + a.eps);
    const DbNorm bn = {mean, invstd, gamma, beta};
    float4 bias4[3], rv[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) bias4[i] = db_bias4(a, c0, i), rv[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (a.res) {
        const __amdgpu_buffer_rsrc_t r_res = rsrc(a.res, ((int64_t)rows - 1) * a.res_ld * 4 + DB_C * 4);
        const unsigned roff = (unsigned)r * (unsigned)a.res_ld * 4u + 4 * c0;
#pragma unroll
        for (int i = 0; i < 3; ++i) rv[i] = ld4(r_res, on ? roff + 4 * DB_K * i : OOB);
    }
    // round trip 2: the neighbour rows + the thread's own pass-through elements; the weight slice behind them (the
    // vector-memory counter retires in order: asked for first, it would hold up every gather).  A later row-block of the
    // workgroup holds the slice already: its gathers go in two rounds of four (no registers for eight rows in flight;
    // hipcc -Rpass-analysis=kernel-resource-usage: 246 VGPRs, 0 bytes of scratch)
    constexpr int ROUND = LOAD_SLICE || !PRODUCT ? DB_W : DB_W / 2;
    float4 z[3];
#pragma unroll
    for (int i = 1; i < 3; ++i) z[i] = ld4(r_src, db_own(own_off, i));
    float4 facc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int n0 = 0; n0 < DB_W; n0 += ROUND) {
        float4 sv[ROUND];
#pragma unroll
        for (int n = 0; n < ROUND; ++n)
            sv[n] = ld4(r_src, on ? rowbase + (unsigned)(nb[n0 + n] >= 0 ? nb[n0 + n] : v) * (DB_C * 4) + 4 * c0 : OOB);
        if (LOAD_SLICE) db_load_slice(bw, a.w_next, wave, lane);
#pragma unroll
        for (int n = 0; n < ROUND; ++n) {
            if (nb[n0 + n] >= 0) { // ELL order == CSR order of the row
                facc.x += wv[n0 + n] * sv[n].x, facc.y += wv[n0 + n] * sv[n].y, facc.z += wv[n0 + n] * sv[n].z, facc.w += wv[n0 + n] * sv[n].w;
            }
        }
    }
    if (tail0 >= 0) { // (the 33-entry poles of 482.obj: entries 8, 9, ... of the row, still in CSR order; -1 pads the end)
        for (int n0 = 0; n0 < DB_TAIL; n0 += 4) {
            const int4 tc4 = *reinterpret_cast<const int4 *>(a.tail_col + (size_t)v * DB_TAIL + n0);
            const float4 tw4 = *reinterpret_cast<const float4 *>(a.tail_val + (size_t)v * DB_TAIL + n0);
            const int tc[4] = {tc4.x, tc4.y, tc4.z, tc4.w};
            const float tw[4] = {tw4.x, tw4.y, tw4.z, tw4.w};
            if (tc[0] < 0) break;
            float4 tv[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) tv[t] = ld4(r_src, (on && tc[t] >= 0) ? rowbase + (unsigned)tc[t] * (DB_C * 4) + 4 * c0 : OOB);
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                if (tc[t] >= 0) {
                    facc.x += tw[t] * tv[t].x, facc.y += tw[t] * tv[t].y, facc.z += tw[t] * tv[t].z, facc.w += tw[t] * tv[t].w;
                }
            }
        }
    }
    z[0] = facc;
    db_add_bias(z, bias4);
    float4 xo[3];
    db_norm_apply(a, bn, z, rv, on, xo); // BatchNorm on the running statistics
    if (a.x_out) {
        const __amdgpu_buffer_rsrc_t r_x = rsrc(a.x_out, op_bytes);
#pragma unroll
        for (int i = 0; i < 3; ++i) st4(r_x, db_own(own_off, i), xo[i]);
    }
    if (!PRODUCT) {
        if (a.w_head) db_head_store(xo, a.w_head, a.s_head, (size_t)r, on, c0); // the coordinate head's raw support
        return;
    }
    // the next layer's product on the tile (rows beyond the last are zero rows of the panel)
    db_to_panel(lds, rl, c0, xo);
    __syncthreads();
    float *stage = lds + RB_PANEL;
    db_product(bw, lds, stage, wave, x, g);
    __syncthreads();
    const __amdgpu_buffer_rsrc_t r_s = rsrc(a.s_out, op_bytes);
    db_store_tile<false>(stage, r_s, [&](int rr) { // (16 consecutive rows = 12 KB contiguous)
        const int row = rb * 16 + rr;
        return row < rows ? (unsigned)row * (DB_C * 4) : OOB;
    });
    // (the next row-block writes the panel, which nobody reads any more; the staging tile only after its first barrier)
}

// logical workgroup -> its run of row-blocks [first, first + count) (zn_stack.hip's q / rem dealing)
__device__ __forceinline__ bool db_deal_row_blocks(int nrb, int nwg, int per_xcd, int &first, int &count)
{
    const int lw = geom::xcd_run_item(blockIdx.x, per_xcd); // contiguous runs per XCD (workgroup w runs on XCD w % 8)
    if (lw >= nwg) return false;
    const int q = nrb / nwg, rem = nrb - q * nwg;
    first = lw * q + (lw < rem ? lw : rem), count = q + (lw < rem ? 1 : 0);
    return true;
}

// (two kernel names: tools and profiles tell the eval launch from the plain one by them)
template <bool PRODUCT>
__global__ __launch_bounds__(DB_THREADS, 2) void di_fwd_kernel(geom_deform_infer a, int nrb, int nwg, int per_xcd)
{
    __shared__ __attribute__((aligned(16))) float lds[RB_PANEL + RB_CST];
    int first, count;
    if (!db_deal_row_blocks(nrb, nwg, per_xcd, first, count)) return;
    DbSlice bw;
    di_row_block<PRODUCT, PRODUCT>(a, first, lds, bw);
    for (int i = 1; i < count; ++i) di_row_block<PRODUCT, false>(a, first + i, lds, bw);
}
template <bool PRODUCT>
__global__ __launch_bounds__(DB_THREADS, 2) void dp_fwd_kernel(geom_deform_plain_fwd a, int nrb, int nwg, int per_xcd)
{
    __shared__ __attribute__((aligned(16))) float lds[RB_PANEL + RB_CST];
    int first, count;
    if (!db_deal_row_blocks(nrb, nwg, per_xcd, first, count)) return;
    DbSlice bw;
    dp_fwd_row_block<PRODUCT, PRODUCT>(a, first, lds, bw);
    for (int i = 1; i < count; ++i) dp_fwd_row_block<PRODUCT, false>(a, first + i, lds, bw);
}

template <bool PRODUCT, bool LOAD_SLICE>
__device__ __forceinline__ void dp_bwd_row_block(const geom_deform_plain_bwd &a, const int rb, float *lds, DbSlice &bw)
{
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int x = lane & 15, g = lane >> 4;
    const int rl = tid >> 4, j = tid & 15;
    const int c0 = 4 * j;
    const int rows = a.b * a.nv;
    const int r = rb * 16 + rl;
    const bool on = r < rows;
    const int mesh = on ? r / a.nv : 0, v = on ? r - mesh * a.nv : 0;
    const int64_t op_bytes = (int64_t)rows * DB_C * 4;
    const unsigned rowbase = (unsigned)mesh * (unsigned)a.nv * (DB_C * 4);
    const unsigned own_off = on ? (unsigned)r * (DB_C * 4) + 4 * c0 : OOB;
    float *stage = lds + RB_PANEL;
    float4 go[3];
    if (PRODUCT) {
        // ---- aggregation backward of the layer above, G = [A^T . dZ_up[:, :64] | dZ_up[:, 64:]], and dX = G . W_up^T
        const __amdgpu_buffer_rsrc_t r_src = rsrc(a.dz_up, op_bytes), r_ds = rsrc(a.ds_up, op_bytes);
        constexpr int ROUND = LOAD_SLICE ? DB_W : DB_W / 2;
        float4 gs[3]; // (stored: the layer above's weight gradient reads it, X^T . G)
#pragma unroll
        for (int i = 1; i < 3; ++i) gs[i] = ld4(r_src, db_own(own_off, i));
        gs[0] = db_row_aggregate<LOAD_SLICE, ROUND>(r_src, on, rowbase, v, c0, a.ell_col_t, a.ell_val_t, a.over_ptr_t, a.over_col_t,
                                                    a.over_val_t, bw, a.wt_up, wave, lane);
#pragma unroll
        for (int i = 0; i < 3; ++i) st4(r_ds, db_own(own_off, i), gs[i]);
        db_to_panel(lds, rl, c0, gs); // (rows beyond the last read zeros: zero rows of the tile)
        __syncthreads();
        db_product(bw, lds, stage, wave, x, g);
        __syncthreads();
        db_load_tile(stage, rl, c0, go);
    } else {
        // ---- the top layer: the caller's gradient, and the coordinate head's backward (db_head_bwd_*)
        const int g_ld = a.g_ld ? a.g_ld : DB_C;
        const __amdgpu_buffer_rsrc_t r_g = rsrc(a.g, ((int64_t)rows - 1) * g_ld * 4 + DB_C * 4);
        const unsigned g_off = on ? ((unsigned)r * (unsigned)g_ld + (unsigned)c0) * 4u : OOB;
#pragma unroll
        for (int i = 0; i < 3; ++i) go[i] = a.g ? ld4(r_g, db_own(g_off, i)) : make_float4(0.f, 0.f, 0.f, 0.f);
        if (a.ds_head) {
            float dsh[3] = {0.f, 0.f, 0.f};
            if (on) {
                const float *src = a.ds_head + (size_t)r * 3;
                dsh[0] = src[0], dsh[1] = src[1], dsh[2] = src[2];
            }
            const __amdgpu_buffer_rsrc_t r_xt = rsrc(a.x_top, op_bytes);
            float *wsum = stage; // [4 waves][192 * 3]
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                const float4 xt = a.dw_head ? ld4(r_xt, db_own(own_off, i)) : make_float4(0.f, 0.f, 0.f, 0.f);
                const float xv[4] = {xt.x, xt.y, xt.z, xt.w};
                float add[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int col = c0 + DB_K * i + e;
                    add[e] = db_head_bwd_input(dsh, a.w_head, col);
                    if (a.dw_head) {
#pragma unroll
                        for (int o = 0; o < 3; ++o) db_head_bwd_weight_rows(xv[e] * dsh[o], wsum, col, o);
                    }
                }
                go[i].x += add[0], go[i].y += add[1], go[i].z += add[2], go[i].w += add[3];
            }
            if (a.dw_head) db_head_bwd_weight_reduce(wsum, a.dw_head, rb); // the ROW-BLOCK's partial
        }
    }
    // ---- this layer: the pending residual gradient, the residual's scale, the ReLU mask (Z > 0: X' loses it under a residual)
    const int g2_ld = a.g2_ld ? a.g2_ld : DB_C;
    const __amdgpu_buffer_rsrc_t r_z = rsrc(a.z, op_bytes), r_g2 = rsrc(a.g2, ((int64_t)rows - 1) * g2_ld * 4 + DB_C * 4);
    const __amdgpu_buffer_rsrc_t r_gr = rsrc(a.grad_res, op_bytes), r_dz = rsrc(a.dz, op_bytes);
    const unsigned g2_off = on ? ((unsigned)r * (unsigned)g2_ld + (unsigned)c0) * 4u : OOB;
    float4 dz[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const float4 zv = a.relu ? ld4(r_z, db_own(own_off, i)) : make_float4(1.f, 1.f, 1.f, 1.f);
        const float4 g2v = a.g2 ? ld4(r_g2, db_own(g2_off, i)) : make_float4(0.f, 0.f, 0.f, 0.f);
        float4 gg = make_float4(go[i].x + g2v.x, go[i].y + g2v.y, go[i].z + g2v.z, go[i].w + g2v.w);
        if (a.has_res) {
            gg.x *= a.scale, gg.y *= a.scale, gg.z *= a.scale, gg.w *= a.scale;
            if (a.grad_res) st4(r_gr, db_own(own_off, i), gg);
        }
        dz[i] = make_float4((on && !(zv.x <= 0.f)) ? gg.x : 0.f, (on && !(zv.y <= 0.f)) ? gg.y : 0.f, (on && !(zv.z <= 0.f)) ? gg.z : 0.f,
                            (on && !(zv.w <= 0.f)) ? gg.w : 0.f);
        st4(r_dz, db_own(own_off, i), dz[i]);
    }
    if (a.colsum) db_colsum(dz, stage, a.colsum, rb, c0); // the row-block's partial of this layer's bias gradient
}

template <bool PRODUCT>
__global__ __launch_bounds__(DB_THREADS, 2) void dp_bwd_kernel(geom_deform_plain_bwd a, int nrb, int nwg, int per_xcd)
{
    __shared__ __attribute__((aligned(16))) float lds[RB_PANEL + RB_CST];
    int first, count;
    if (!db_deal_row_blocks(nrb, nwg, per_xcd, first, count)) return;
    DbSlice bw;
    dp_bwd_row_block<PRODUCT, PRODUCT>(a, first, lds, bw);
    for (int i = 1; i < count; ++i) {
        __syncthreads(); // (the staging tile: the column sums of the row-block before are read)
        dp_bwd_row_block<PRODUCT, false>(a, first + i, lds, bw);
    }
}

// ---- training batches of 17 .. GEOM_DEFORM_WIDE_MAX_B meshes (geom_deform_layer_wide_{fwd,bwd}_f32): one launch per hidden
// layer and direction, still one workgroup per VERTEX; the vertex's b rows are T = ceil(b / 16) <= 4 row tiles of the matrix
// core (tile t, tile row rl = mesh 16 t + rl; rows at or beyond b are zero rows of the panel and store nothing).
//
// Schedule of a workgroup (forward; the backward mirrors it):
//   1. the T tiles' gathers one after the other through db_aggregate (the plain launch's order: same bits), no weight slice
//      live yet -- a pole's 32 tail rows per tile need the registers; Z leaves for z_out and STAYS in registers (12 floats per
//      tile, 48 at most) for both statistics passes;
//   2. the wave's weight slice (144 registers) is requested ONCE, in front of the statistics, and serves all T products;
//   3. the vertex's statistics over all b * 192 values: per thread over its tiles in tile order, then db_sum2 (mean; then the
//      centred second moment) -- the tiles meet inside the workgroup, in a fixed order, no atomics;
//   4. per tile: BatchNorm + ReLU + residual -> x_out, the panel, the product, s_out (the residual of tile t + 1 is requested
//      before the product of tile t).
// Backward: 1. the T tiles' gathers of dZ_up -> G (ds_up), kept in registers; 2. the slice; 3. per tile G . W_up^T through the
// panel, the product's rows replace G in the registers (the slice is dead from here on); 4. Z and the second gradient per tile,
// mask + the two sums over all tiles (db_sum2); 5. dZ per tile, the column sums over tiles, then lanes, then waves.
constexpr int DBW_TILES = GEOM_DEFORM_WIDE_MAX_B / 16;

template <bool PRODUCT>
__global__ __launch_bounds__(DB_THREADS, 2) void dbw_fwd_kernel(geom_deform_fwd a)
{
    __shared__ __attribute__((aligned(16))) float lds[RB_PANEL + RB_CST + DB_RED];
    const int v = db_vertex(blockIdx.x, a.vpx, a.nv);
    if (v < 0) return;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int x = lane & 15, g = lane >> 4;
    const int rl = tid >> 4, j = tid & 15;
    const int c0 = 4 * j;
    const int tiles = (a.b + 15) >> 4;
    const int64_t op_bytes = (int64_t)a.b * a.nv * DB_C * 4;
    const __amdgpu_buffer_rsrc_t r_src = rsrc(a.s_in, op_bytes);
    const __amdgpu_buffer_rsrc_t r_z = rsrc(a.z_out, op_bytes), r_x = rsrc(a.x_out, op_bytes);
    const __amdgpu_buffer_rsrc_t r_res = rsrc(a.res, ((int64_t)a.b * a.nv - 1) * a.res_ld * 4 + DB_C * 4);
    // byte offset of the thread's first float4 of tile t in a [b, nv, 192] operand (OOB: a row at or beyond b)
    auto own = [&](int t) {
        const int mesh = 16 * t + rl;
        return mesh < a.b ? ((unsigned)mesh * (unsigned)a.nv + (unsigned)v) * (DB_C * 4) + 4 * c0 : OOB;
    };
    auto residual = [&](int t, float4 (&rv)[3]) {
        const int mesh = 16 * t + rl;
        const unsigned roff = ((unsigned)mesh * (unsigned)a.nv + (unsigned)v) * (unsigned)a.res_ld * 4u + 4 * c0;
#pragma unroll
        for (int i = 0; i < 3; ++i) rv[i] = a.res ? ld4(r_res, mesh < a.b ? roff + 4 * DB_K * i : OOB) : make_float4(0.f, 0.f, 0.f, 0.f);
    };
    const float gamma = a.bn_w ? a.bn_w[v] : 1.f, beta = a.bn_b ? a.bn_b[v] : 0.f;
    const bool updates = a.training && tid == 0;
    const float old_mean = (updates && a.run_mean) ? a.run_mean[v] : 0.f, old_var = (updates && a.run_var) ? a.run_var[v] : 0.f;
    float4 bias4[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) bias4[i] = db_bias4(a, c0, i);
    const DbTable tb = db_table(v, a.ell_col, a.ell_val, a.tail_col, a.tail_val, lane);

    // ---- 1. the tiles' aggregations
    float4 z[DBW_TILES][3];
    DbSlice bw;
#pragma unroll
    for (int t = 0; t < DBW_TILES; ++t) {
#pragma unroll
        for (int i = 0; i < 3; ++i) z[t][i] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (t < tiles) {
            const int mesh = 16 * t + rl;
            const unsigned rowbase = (unsigned)mesh * (unsigned)a.nv * (DB_C * 4);
            z[t][0] = db_aggregate<false, false>(r_src, mesh < a.b, rowbase, v, c0, tb, &z[t][1], bw, nullptr, wave, lane);
            db_add_bias(z[t], bias4);
#pragma unroll
            for (int i = 0; i < 3; ++i)
                if (a.z_out) st4(r_z, db_own(own(t), i), z[t][i]);
        }
    }
    // ---- 2. the weight slice for all tiles, and the first tile's residual, under the statistics
    __builtin_amdgcn_sched_barrier(0);
    if (PRODUCT) db_load_slice(bw, a.w_next, wave, lane);
    float4 rvn[3];
    residual(0, rvn);
    __builtin_amdgcn_sched_barrier(0);

    // ---- 3. BatchNorm1d(verts): one statistic per vertex over its b * 192 values (two-pass: mean, then the centred second moment)
    float *red = lds + RB_PANEL + RB_CST;
    const int n = a.b * DB_C;
    DbNorm bn;
    if (a.training) {
        float s = 0.f, dummy = 0.f;
#pragma unroll
        for (int t = 0; t < DBW_TILES; ++t) {
            const float st = db_row_sum(z[t]);
            if (16 * t + rl < a.b) s += st;
        }
        db_sum2(s, dummy, red);
        bn.mean = s / n;
        float q = 0.f;
#pragma unroll
        for (int t = 0; t < DBW_TILES; ++t) {
            const float qt = db_row_centred_sq(z[t], bn.mean);
            if (16 * t + rl < a.b) q += qt;
        }
        dummy = 0.f;
        db_sum2(q, dummy, red);
        bn.invstd = db_publish_stats(a, v, n, bn.mean, q, old_mean, old_var);
    } else {
        bn.mean = a.run_mean[v];
        bn.invstd = 1.f / sqrtf(a.run_var[v] + a.eps);
    }
    bn.gamma = gamma, bn.beta = beta;

    // ---- 4. the tiles' outputs and products
    float *stage = lds + RB_PANEL;
    const __amdgpu_buffer_rsrc_t r_s = rsrc(a.s_out, op_bytes);
#pragma unroll
    for (int t = 0; t < DBW_TILES; ++t) {
        if (t < tiles) {
            const bool mesh_on = 16 * t + rl < a.b;
            float4 rv[3];
#pragma unroll
            for (int i = 0; i < 3; ++i) rv[i] = rvn[i];
            if (t + 1 < tiles) residual(t + 1, rvn);
            float4 xo[3];
            db_norm_apply(a, bn, z[t], rv, mesh_on, xo);
#pragma unroll
            for (int i = 0; i < 3; ++i) st4(r_x, db_own(own(t), i), xo[i]);
            if (!PRODUCT) {
                // the coordinate head's product inside the last hidden layer's launch
                if (a.w_head && a.s_head) db_head_store(xo, a.w_head, a.s_head, (size_t)(16 * t + rl) * a.nv + v, mesh_on, c0);
            } else {
                // (the panel's readers and the staging tile's are behind the previous tile's two barriers)
                db_to_panel(lds, rl, c0, xo);
                __syncthreads();
                db_product(bw, lds, stage, wave, x, g);
                __syncthreads();
                db_store_tile<false>(stage, r_s, [&](int r) {
                    const int mesh = 16 * t + r;
                    return mesh < a.b ? ((unsigned)mesh * (unsigned)a.nv + (unsigned)v) * (DB_C * 4) : OOB;
                });
                __syncthreads(); // (the staging tile is free for the next tile's product)
            }
        }
    }
}

template <bool PRODUCT>
__global__ __launch_bounds__(DB_THREADS, 2) void dbw_bwd_kernel(geom_deform_bwd a)
{
    __shared__ __attribute__((aligned(16))) float lds[RB_PANEL + RB_CST + DB_RED];
    const int v = db_vertex(blockIdx.x, a.vpx, a.nv);
    if (v < 0) return;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int x = lane & 15, g = lane >> 4;
    const int rl = tid >> 4, j = tid & 15;
    const int c0 = 4 * j;
    const int tiles = (a.b + 15) >> 4;
    const int64_t op_bytes = (int64_t)a.b * a.nv * DB_C * 4;
    const int g_ld = a.g_ld ? a.g_ld : DB_C, g2_ld = a.g2_ld ? a.g2_ld : DB_C;
    const __amdgpu_buffer_rsrc_t r_z = rsrc(a.z, op_bytes);
    const __amdgpu_buffer_rsrc_t r_g2 = rsrc(a.g2, ((int64_t)a.b * a.nv - 1) * g2_ld * 4 + DB_C * 4);
    const __amdgpu_buffer_rsrc_t r_g = rsrc(a.g, ((int64_t)a.b * a.nv - 1) * g_ld * 4 + DB_C * 4);
    const __amdgpu_buffer_rsrc_t r_gr = rsrc(a.grad_res, op_bytes), r_dz = rsrc(a.dz, op_bytes);
    // byte offset of the thread's float4 i of tile t in a [b, nv, ld] operand (OOB: a row at or beyond b)
    auto at = [&](int t, int i, int ld) {
        const int mesh = 16 * t + rl;
        return mesh < a.b ? (((unsigned)mesh * (unsigned)a.nv + (unsigned)v) * (unsigned)ld + (unsigned)(c0 + DB_K * i)) * 4u : OOB;
    };
    const float mean = a.save_mean[v], invstd = a.save_invstd[v];
    const float gamma = a.bn_w ? a.bn_w[v] : 1.f, beta = a.bn_b ? a.bn_b[v] : 0.f;
    float *stage = lds + RB_PANEL;
    float4 go[DBW_TILES][3];
#pragma unroll
    for (int t = 0; t < DBW_TILES; ++t)
#pragma unroll
        for (int i = 0; i < 3; ++i) go[t][i] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (PRODUCT) {
        // ---- 1. aggregation backward of the layer above, tile by tile: G = [A^T . dZ_up[:, :64] | dZ_up[:, 64:]]
        const __amdgpu_buffer_rsrc_t r_src = rsrc(a.dz_up, op_bytes), r_ds = rsrc(a.ds_up, op_bytes);
        const DbTable tb = db_table(v, a.ell_col_t, a.ell_val_t, a.tail_col_t, a.tail_val_t, lane);
        DbSlice bw;
#pragma unroll
        for (int t = 0; t < DBW_TILES; ++t) {
            if (t < tiles) {
                const int mesh = 16 * t + rl;
                const unsigned rowbase = (unsigned)mesh * (unsigned)a.nv * (DB_C * 4);
                go[t][0] = db_aggregate<false, false>(r_src, mesh < a.b, rowbase, v, c0, tb, &go[t][1], bw, nullptr, wave, lane);
#pragma unroll
                for (int i = 0; i < 3; ++i) st4(r_ds, at(t, i, DB_C), go[t][i]); // the layer above's weight gradient reads it
            }
        }
        // ---- 2. the slice of W_up^T, once for all tiles; 3. dX = G . W_up^T
        __builtin_amdgcn_sched_barrier(0);
        db_load_slice(bw, a.wt_up, wave, lane);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int t = 0; t < DBW_TILES; ++t) {
            if (t < tiles) {
                db_to_panel(lds, rl, c0, go[t]); // (rows beyond the batch read zeros: zero rows of the tile)
                __syncthreads();
                db_product(bw, lds, stage, wave, x, g);
                __syncthreads();
                db_load_tile(stage, rl, c0, go[t]);
                __syncthreads(); // (the staging tile is free for the next tile's product)
            }
        }
    } else {
#pragma unroll
        for (int t = 0; t < DBW_TILES; ++t)
            if (t < tiles && a.g) {
#pragma unroll
                for (int i = 0; i < 3; ++i) go[t][i] = ld4(r_g, at(t, i, g_ld));
            }
        if (a.ds_head) {
            // ---- the coordinate head inside the first backward launch (db_head_bwd_*): its input gradient joins g; the vertex's
            // partial of its weight gradient: per thread over its tiles in tile order, then the wave's rows, then the waves
            const __amdgpu_buffer_rsrc_t r_xt = rsrc(a.x_top, op_bytes);
            float *wsum = lds + RB_PANEL; // [4 waves][192 * 3]
            float part[3][4][3];
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int e = 0; e < 4; ++e)
#pragma unroll
                    for (int o = 0; o < 3; ++o) part[i][e][o] = 0.f;
#pragma unroll
            for (int t = 0; t < DBW_TILES; ++t) {
                if (t < tiles) {
                    const int mesh = 16 * t + rl;
                    float dsh[3] = {0.f, 0.f, 0.f};
                    if (mesh < a.b) {
                        const float *src = a.ds_head + ((size_t)mesh * a.nv + v) * 3;
                        dsh[0] = src[0], dsh[1] = src[1], dsh[2] = src[2];
                    }
#pragma unroll
                    for (int i = 0; i < 3; ++i) {
                        const float4 xt = a.dw_head ? ld4(r_xt, at(t, i, DB_C)) : make_float4(0.f, 0.f, 0.f, 0.f);
                        const float xv[4] = {xt.x, xt.y, xt.z, xt.w};
                        float add[4];
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            add[e] = db_head_bwd_input(dsh, a.w_head, c0 + DB_K * i + e);
#pragma unroll
                            for (int o = 0; o < 3; ++o) part[i][e][o] += xv[e] * dsh[o];
                        }
                        go[t][i].x += add[0], go[t][i].y += add[1], go[t][i].z += add[2], go[t][i].w += add[3];
                    }
                }
            }
            if (a.dw_head) {
#pragma unroll
                for (int i = 0; i < 3; ++i)
#pragma unroll
                    for (int e = 0; e < 4; ++e)
#pragma unroll
                        for (int o = 0; o < 3; ++o) db_head_bwd_weight_rows(part[i][e][o], wsum, c0 + DB_K * i + e, o);
                db_head_bwd_weight_reduce(wsum, a.dw_head, v);
            }
        }
    }
    // ---- 4. this layer: residual scale, ReLU mask, the two sums of the BatchNorm backward over all tiles
    float sum_g = 0.f, sum_gx = 0.f;
    float4 xh[DBW_TILES][3];
#pragma unroll
    for (int t = 0; t < DBW_TILES; ++t) {
#pragma unroll
        for (int i = 0; i < 3; ++i) xh[t][i] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (t < tiles) {
            const bool mesh_on = 16 * t + rl < a.b;
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                const float4 zv = ld4(r_z, at(t, i, DB_C));
                const float4 s = a.g2 ? ld4(r_g2, at(t, i, g2_ld)) : make_float4(0.f, 0.f, 0.f, 0.f);
                db_bn_bwd_elems(a, mean, invstd, gamma, beta, mesh_on, zv, go[t][i], s, xh[t][i], sum_g, sum_gx, r_gr, at(t, i, DB_C));
            }
        }
    }
    float *red = lds + RB_PANEL + RB_CST;
    db_sum2(sum_g, sum_gx, red);
    db_publish_bn_grads(a, v, sum_g, sum_gx);
    // ---- 5. dZ, and the vertex's column sums of dZ over its meshes (per thread over its tiles, the wave's rows, the waves)
    const int n = a.b * DB_C;
    const float kk = gamma * invstd, mg = sum_g / n, mgx = sum_gx / n;
    float4 cs[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) cs[i] = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int t = 0; t < DBW_TILES; ++t) {
        if (t < tiles) {
            const bool mesh_on = 16 * t + rl < a.b;
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                const float4 dz = db_bn_bwd_dz4(kk, go[t][i], xh[t][i], mg, mgx, mesh_on);
                st4(r_dz, at(t, i, DB_C), dz);
                cs[i].x += dz.x, cs[i].y += dz.y, cs[i].z += dz.z, cs[i].w += dz.w;
            }
        }
    }
    if (a.colsum) db_colsum(cs, stage, a.colsum, v, c0);
}

inline bool db_aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

// max_b: 16 for the launches of one row tile per vertex, GEOM_DEFORM_WIDE_MAX_B for the wide ones
int db_check_shape(int b, int nv, int c, int k, int ell_w, int max_b = 16)
{
    if (b < 0 || nv < 0 || c <= 0 || k < 0) return GEOM_EINVAL;
    if (c != DB_C || k != DB_K || ell_w != DB_W || b > max_b) return GEOM_EUNSUPPORTED;
    if ((int64_t)b * nv * DB_C >= (1LL << 29)) return GEOM_EUNSUPPORTED; // 32-bit byte offsets
    return 0;
}

// What geom_deform_fwd and geom_deform_infer ask alike of the operands they have in common; every failure is GEOM_EINVAL.
template <typename Args>
bool db_fwd_operands_ok(const Args &a)
{
    if (!a.s_in || !a.ell_col || !a.ell_val) return false;
    if (a.w_next && !a.s_out) return false;
    if ((a.w_head != nullptr) != (a.s_head != nullptr) || (a.w_head && a.w_next)) return false; // the head rides in the launch without a product
    if (a.tail_col && !a.tail_val) return false;
    if (a.res && a.res_ld < DB_C) return false; // (any pitch: a column slice of the block's 1155-wide input is read in place)
    return db_aligned16(a.s_in) && db_aligned16(a.ell_col) && db_aligned16(a.ell_val) && db_aligned16(a.x_out) && db_aligned16(a.s_out) &&
           db_aligned16(a.bias) && !((uintptr_t)a.res & 3) && db_aligned16(a.w_next);
}

// The operands of ONE forward layer of a non-empty shape that passed db_check_shape; fills in what the kernels read beside them.
int db_check_fwd(geom_deform_fwd &a)
{
    if (!db_fwd_operands_ok(a) || !a.x_out || !db_aligned16(a.z_out)) return GEOM_EINVAL;
    if (a.training ? (!a.save_mean || !a.save_invstd) : (!a.run_mean || !a.run_var)) return GEOM_EINVAL;
    if (a.res && (int64_t)a.b * a.nv * a.res_ld >= (1LL << 29)) return GEOM_EUNSUPPORTED; // 32-bit byte offsets of the residual
    if (!a.res) a.scale = 1.f;
    a.vpx = (a.nv + 7) / 8;
    return 0;
}

// ... and of one backward layer.  The first failing check decides the code.
int db_check_bwd(geom_deform_bwd &a)
{
    if (!a.z || !a.save_mean || !a.save_invstd || !a.dz) return GEOM_EINVAL;
    const bool product = a.dz_up != nullptr;
    if (product ? (!a.ell_col_t || !a.ell_val_t || !a.ds_up || !a.wt_up) : (!a.g && !a.ds_head)) return GEOM_EINVAL;
    if (a.ds_head && (product || !a.w_head || (a.dw_head && !a.x_top) || !db_aligned16(a.x_top))) return GEOM_EINVAL;
    if (a.tail_col_t && !a.tail_val_t) return GEOM_EINVAL;
    if ((a.g_ld && a.g_ld < DB_C) || (a.g2_ld && a.g2_ld < DB_C)) return GEOM_EINVAL;
    if ((int64_t)a.b * a.nv * (a.g_ld > a.g2_ld ? a.g_ld : a.g2_ld) >= (1LL << 29)) return GEOM_EUNSUPPORTED;
    if (!db_aligned16(a.dz_up) || !db_aligned16(a.ell_col_t) || !db_aligned16(a.ell_val_t) || !db_aligned16(a.ds_up) || ((uintptr_t)a.g & 3) ||
        ((uintptr_t)a.g2 & 3) || !db_aligned16(a.z) || !db_aligned16(a.grad_res) || !db_aligned16(a.dz) || !db_aligned16(a.colsum) ||
        !db_aligned16(a.wt_up))
        return GEOM_EINVAL;
    if (!a.has_res) a.scale = 1.f;
    a.vpx = (a.nv + 7) / 8;
    return 0;
}

// whether the layer's launch carries a product (forward: the next layer's; backward: the input gradient of the layer above)
inline bool db_has_product(const geom_deform_fwd &a) { return a.w_next != nullptr; }
inline bool db_has_product(const geom_deform_bwd &a) { return a.dz_up != nullptr; }
inline int db_check_layer(geom_deform_fwd &a) { return db_check_fwd(a); }
inline int db_check_layer(geom_deform_bwd &a) { return db_check_bwd(a); }

template <typename Args, void (*WITH_PRODUCT)(Args), void (*WITHOUT)(Args)>
int db_launch_layer(const Args *args, void *stream, int min_b, int max_b)
{
    if (!args) return GEOM_EINVAL;
    Args a = *args;
    int code = db_check_shape(a.b, a.nv, a.c, a.k, a.ell_w, max_b);
    if (code) return code;
    if (a.b == 0 || a.nv == 0) return 0;
    if (a.b <= min_b) return GEOM_EUNSUPPORTED;
    if ((code = db_check_layer(a))) return code;
    const dim3 grid(8 * a.vpx), block(DB_THREADS);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (db_has_product(a)) hipLaunchKernelGGL(WITH_PRODUCT, grid, block, 0, s, a);
    else hipLaunchKernelGGL(WITHOUT, grid, block, 0, s, a);
    return geom::launch_status();
}

// The grid of a row-block launch (the eval and the two plain entry points): ceil(b nv / 16) row-blocks dealt to at most DI_WGS
// logical workgroups, in runs per XCD.  launch(grid, block, nrb, nwg, per_xcd) enqueues the kernel.
template <typename Args, typename Launch>
int db_launch_row_blocks(const Args &l, Launch launch)
{
    const int nrb = (l.b * l.nv + 15) / 16;
    const int nwg = nrb < DI_WGS ? nrb : DI_WGS, per_xcd = (nwg + 7) / 8;
    launch(dim3(8 * per_xcd), dim3(DB_THREADS), nrb, nwg, per_xcd);
    return geom::launch_status();
}

} // namespace

#ifdef DB_PROBE_STAMPS
extern "C" int geom_db_probe_read(unsigned long long *dst, int n)
{
    return (int)hipMemcpyFromSymbol(dst, HIP_SYMBOL(db_stamps), sizeof(unsigned long long) * n, 0, hipMemcpyDeviceToHost);
}
#endif

// The four launches of ONE layer: plain (a vertex's 1 <= b <= 16 rows are one row tile) and wide (17 <= b <=
// GEOM_DEFORM_WIDE_MAX_B: ceil(b / 16) tiles), forward and backward, have one set of checks in one order -- the first failing
// one decides the code -- and one launch shape.  A batch outside the entry's window (min_b, max_b] belongs to the other entry
// point: GEOM_EUNSUPPORTED.
extern "C" int geom_deform_layer_fwd_f32(const geom_deform_fwd *args, void *stream)
{
    return db_launch_layer<geom_deform_fwd, db_fwd_kernel<true>, db_fwd_kernel<false>>(args, stream, 0, 16);
}

extern "C" int geom_deform_layer_bwd_f32(const geom_deform_bwd *args, void *stream)
{
    return db_launch_layer<geom_deform_bwd, db_bwd_kernel<true>, db_bwd_kernel<false>>(args, stream, 0, 16);
}

extern "C" int geom_deform_layer_wide_fwd_f32(const geom_deform_fwd *args, void *stream)
{
    return db_launch_layer<geom_deform_fwd, dbw_fwd_kernel<true>, dbw_fwd_kernel<false>>(args, stream, 16, GEOM_DEFORM_WIDE_MAX_B);
}

extern "C" int geom_deform_layer_wide_bwd_f32(const geom_deform_bwd *args, void *stream)
{
    return db_launch_layer<geom_deform_bwd, dbw_bwd_kernel<true>, dbw_bwd_kernel<false>>(args, stream, 16, GEOM_DEFORM_WIDE_MAX_B);
}

// `count` backward layers in execution order (layers[0] = the top layer, read from memory: dz_up == NULL; layers[t].dz_up ==
// layers[t - 1].dz for t >= 1) in ONE launch; results = those of the separate geom_deform_layer_bwd_f32 calls, bit for bit.
// done: as for geom_deform_chain_fwd_f32 (its own nv * 32 zeroed ints).  ds_first (may be NULL): also the aggregation backward of
// the last step's dZ, [A^T . dZ[:, :64] | dZ[:, 64:]] -> ds_first [b,nv,192] (the support gradient of the chain's first layer;
// the bits of geom_zn_gcn_aggregate_ell_bwd_f32 without activation), as a last hand-off of the same launch.
extern "C" int geom_deform_chain_bwd_f32(int count, const geom_deform_bwd *layers, int *done, float *ds_first, void *stream)
{
    if (count <= 0 || count > GEOM_DEFORM_CHAIN_MAX || !layers || !done || ((uintptr_t)done & 127)) return GEOM_EINVAL;
    if (ds_first && (count < 2 || !db_aligned16(ds_first))) return GEOM_EINVAL; // (the transposed tables come with layers[1])
    DbBwdChain c{};
    for (int l = 0; l < count; ++l) {
        geom_deform_bwd a = layers[l];
        int code = db_check_shape(a.b, a.nv, a.c, a.k, a.ell_w);
        if (code) return code;
        if (a.b != layers[0].b || a.nv != layers[0].nv) return GEOM_EINVAL;
        const bool product = a.dz_up != nullptr;
        if (product != (l > 0)) return GEOM_EINVAL;                                   // only the top layer reads its gradient from memory
        if (product && a.dz_up != layers[l - 1].dz) return GEOM_EINVAL;               // a chain
        if (product && l > 1 && (a.ell_col_t != layers[1].ell_col_t || a.ell_val_t != layers[1].ell_val_t ||
                                 a.tail_col_t != layers[1].tail_col_t || a.tail_val_t != layers[1].tail_val_t))
            return GEOM_EINVAL;
        if ((code = db_check_bwd(a))) return code;                                    // (its 2^29 limit answers before the next check)
        for (int e = 0; e < l; ++e)
            if (layers[e].dz == a.dz) return GEOM_EINVAL;                              // (every step its own dZ: neighbours read it a step later)
        c.layer[l] = a;
    }
    if (layers[0].b == 0 || layers[0].nv == 0) return 0;
    if (!geom_deform_chain_fits(layers[0].nv)) return GEOM_EUNSUPPORTED;
    c.count = count, c.done = done, c.ds_first = ds_first;
    hipLaunchKernelGGL(db_bwd_chain_kernel, dim3(8 * c.layer[0].vpx), dim3(DB_THREADS), 0, static_cast<hipStream_t>(stream), c);
    return geom::launch_status();
}

// One eval-mode hidden layer over b >= 1 meshes (see di_row_block).  Every invalid argument is GEOM_EINVAL, decided on the host
// before anything is enqueued.
extern "C" int geom_deform_infer_fwd_f32(const geom_deform_infer *args, void *stream)
{
    if (!args) return GEOM_EINVAL;
    const geom_deform_infer a = *args;
    if (a.b < 1 || a.nv < 1 || a.c != DB_C || a.k != DB_K || a.ell_w != DB_W) return GEOM_EINVAL;
    if ((int64_t)a.b * a.nv * DB_C >= (1LL << 29)) return GEOM_EINVAL; // 32-bit byte offsets
    if (!db_fwd_operands_ok(a) || !a.run_mean || !a.run_var) return GEOM_EINVAL;
    if (!a.w_next && (a.s_out || (!a.x_out && !a.s_head))) return GEOM_EINVAL;                       // no product: no s_out, and something to write
    if (a.tail_val && !a.tail_col) return GEOM_EINVAL;
    if (a.res && (int64_t)a.b * a.nv * a.res_ld >= (1LL << 29)) return GEOM_EINVAL;
    if (!db_aligned16(a.tail_col) || !db_aligned16(a.tail_val)) return GEOM_EINVAL;
    geom_deform_infer l = a;
    if (!l.res) l.scale = 1.f;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return db_launch_row_blocks(l, [&](dim3 grid, dim3 block, int nrb, int nwg, int per_xcd) {
        if (l.w_next) hipLaunchKernelGGL((di_fwd_kernel<true>), grid, block, 0, s, l, nrb, nwg, per_xcd);
        else hipLaunchKernelGGL((di_fwd_kernel<false>), grid, block, 0, s, l, nrb, nwg, per_xcd);
    });
}

namespace {
// what the two plain entry points ask alike: the shape, and a table with its values / an overflow list with all three arrays
bool dp_shape_and_tables_ok(int b, int nv, int c, int k, const int *ell_col, const float *ell_val, const int *over_ptr, const int *over_col,
                            const float *over_val)
{
    if (b < 1 || nv < 1 || c != DB_C || k != DB_K) return false;
    if ((int64_t)b * nv * DB_C >= (1LL << 29)) return false; // 32-bit byte offsets
    if ((ell_col != nullptr) != (ell_val != nullptr)) return false;
    if ((over_col || over_val) && !over_ptr) return false;
    if (over_ptr && (!over_col || !over_val)) return false;
    return db_aligned16(ell_col) && db_aligned16(ell_val) && !((uintptr_t)over_ptr & 3) && !((uintptr_t)over_col & 3) && !((uintptr_t)over_val & 3);
}
// a row pitch in floats (0 = 192) of an operand read in place
bool dp_pitch_ok(const void *p, int ld, int b, int nv)
{
    if (ld && ld < DB_C) return false;
    return !((uintptr_t)p & 3) && (int64_t)b * nv * (ld ? ld : DB_C) < (1LL << 29);
}
} // namespace

// One hidden layer of the BatchNorm-free block, forward (see dp_fwd_row_block).  Every invalid argument is GEOM_EINVAL, decided
// on the host before anything is enqueued.
extern "C" int geom_deform_plain_fwd_f32(const geom_deform_plain_fwd *args, void *stream)
{
    if (!args) return GEOM_EINVAL;
    geom_deform_plain_fwd l = *args;
    if (!dp_shape_and_tables_ok(l.b, l.nv, l.c, l.k, l.ell_col, l.ell_val, l.over_ptr, l.over_col, l.over_val)) return GEOM_EINVAL;
    if (!l.s_in || !l.ell_col) return GEOM_EINVAL;
    if ((l.w_next != nullptr) != (l.s_out != nullptr)) return GEOM_EINVAL;
    if ((l.w_head != nullptr) != (l.s_head != nullptr) || (l.w_head && l.w_next)) return GEOM_EINVAL; // the head rides without a product
    if (!l.z_out && !l.x_out && !l.s_out && !l.s_head) return GEOM_EINVAL;                            // nothing to write
    if (l.res && (l.res_ld < DB_C || !dp_pitch_ok(l.res, l.res_ld, l.b, l.nv))) return GEOM_EINVAL;
    if (!db_aligned16(l.s_in) || !db_aligned16(l.bias) || !db_aligned16(l.z_out) || !db_aligned16(l.x_out) || !db_aligned16(l.s_out) ||
        !db_aligned16(l.w_next) || ((uintptr_t)l.w_head & 3) || ((uintptr_t)l.s_head & 3))
        return GEOM_EINVAL;
    if (!l.res) l.scale = 1.f;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return db_launch_row_blocks(l, [&](dim3 grid, dim3 block, int nrb, int nwg, int per_xcd) {
        if (l.w_next) hipLaunchKernelGGL((dp_fwd_kernel<true>), grid, block, 0, s, l, nrb, nwg, per_xcd);
        else hipLaunchKernelGGL((dp_fwd_kernel<false>), grid, block, 0, s, l, nrb, nwg, per_xcd);
    });
}

// ... and backward (see dp_bwd_row_block): with dz_up the aggregation backward and input-gradient product of the layer above,
// without it the top layer (the caller's gradient, the coordinate head).
extern "C" int geom_deform_plain_bwd_f32(const geom_deform_plain_bwd *args, void *stream)
{
    if (!args) return GEOM_EINVAL;
    geom_deform_plain_bwd l = *args;
    if (!dp_shape_and_tables_ok(l.b, l.nv, l.c, l.k, l.ell_col_t, l.ell_val_t, l.over_ptr_t, l.over_col_t, l.over_val_t)) return GEOM_EINVAL;
    if (!l.dz || (l.relu && !l.z)) return GEOM_EINVAL;
    const bool product = l.dz_up != nullptr;
    if (product ? (!l.ell_col_t || !l.ds_up || !l.wt_up || l.g) : (l.ds_up || l.wt_up || (!l.g && !l.ds_head))) return GEOM_EINVAL;
    if (l.ds_head ? (product || !l.w_head || (l.dw_head && !l.x_top)) : (l.dw_head != nullptr)) return GEOM_EINVAL;
    if (!dp_pitch_ok(l.g, l.g_ld, l.b, l.nv) || !dp_pitch_ok(l.g2, l.g2_ld, l.b, l.nv)) return GEOM_EINVAL;
    if (!db_aligned16(l.dz_up) || !db_aligned16(l.ds_up) || !db_aligned16(l.wt_up) || !db_aligned16(l.z) || !db_aligned16(l.grad_res) ||
        !db_aligned16(l.dz) || !db_aligned16(l.colsum) || !db_aligned16(l.x_top) || !db_aligned16(l.dw_head) || ((uintptr_t)l.ds_head & 3) ||
        ((uintptr_t)l.w_head & 3))
        return GEOM_EINVAL;
    if (!l.has_res) l.scale = 1.f;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return db_launch_row_blocks(l, [&](dim3 grid, dim3 block, int nrb, int nwg, int per_xcd) {
        if (product) hipLaunchKernelGGL((dp_bwd_kernel<true>), grid, block, 0, s, l, nrb, nwg, per_xcd);
        else hipLaunchKernelGGL((dp_bwd_kernel<false>), grid, block, 0, s, l, nrb, nwg, per_xcd);
    });
}

// fwd[l] / bwd[l] (each count x 36 864 floats, either may be NULL) = the register-slice order of w[l] / w[l]^T that
// geom_deform_layer_fwd_f32 (w_next) / geom_deform_layer_bwd_f32 (wt_up) read; w = HOST array of count <= GEOM_DEFORM_MAX_PACK
// device pointers to [192,192] row-major matrices.  One launch for all layers of a block, once per step.
extern "C" int geom_deform_pack_weights_f32(int count, const float *const *w, float *fwd, float *bwd, void *stream)
{
    return geom_deform_pack_weights_zero_f32(count, w, fwd, bwd, nullptr, 0, stream);
}

// ... and `zero_words` 4-byte words at `zero` cleared by the same launch (the counters of the step's chain launches)
extern "C" int geom_deform_pack_weights_zero_f32(int count, const float *const *w, float *fwd, float *bwd, int *zero, int zero_words,
                                                 void *stream)
{
    if (count < 0 || count > GEOM_DEFORM_MAX_PACK || zero_words < 0 || (zero_words > 0 && !zero)) return GEOM_EINVAL;
    if (count == 0 || (!fwd && !bwd)) count = 0;
    if (count == 0 && zero_words == 0) return 0;
    if (count && (!w || !db_aligned16(fwd) || !db_aligned16(bwd))) return GEOM_EINVAL;
    DbPackArgs a{};
    for (int i = 0; i < count; ++i) {
        if (!w[i] || ((uintptr_t)w[i] & 3)) return GEOM_EINVAL;
        a.w[i] = w[i];
    }
    a.fwd = fwd, a.bwd = bwd, a.count = count;
    const int total = count * 2 * DB_C * DB_C;
    a.pack_blocks = (total + 255) / 256, a.zero = zero, a.zero_words = zero_words;
    hipLaunchKernelGGL(db_pack_kernel, dim3(a.pack_blocks + (zero_words + 255) / 256), dim3(256), 0, static_cast<hipStream_t>(stream), a);
    return geom::launch_status();
}

// Whether a chain launch over nv vertices can run on the current device: every workgroup must be resident at once (a
// workgroup waits for its neighbours' INSIDE the launch).
extern "C" int geom_deform_chain_fits(int nv)
{
    if (nv <= 0) return 0;
    static int slots[geom::MAX_DEVICES] = {0}; // per device: the occupancy query is not free
    const geom::DeviceFacts *dev = geom::device_facts();
    if (!dev) return 0;
    int &have = slots[dev->device];
    if (!have) {
        int per_cu = 0, per_cu_b = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, db_fwd_chain_kernel, DB_THREADS, 0) != hipSuccess ||
            hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu_b, db_bwd_chain_kernel, DB_THREADS, 0) != hipSuccess)
            return 0;
        per_cu = per_cu < per_cu_b ? per_cu : per_cu_b;
        have = per_cu > 0 ? per_cu * dev->compute_units : -1;
    }
    return have >= 8 * ((nv + 7) / 8);
}

// `count` consecutive layers (layers[l + 1].s_in == layers[l].s_out, all but possibly the last with a product) in ONE launch;
// results = those of `count` geom_deform_layer_fwd_f32 calls, bit for bit.  done: nv * 32 ints, ZERO on entry
// (geom_deform_pack_weights_zero_f32 of the same step), 128-byte aligned.  GEOM_EUNSUPPORTED when the launch does not fit the
// device (geom_deform_chain_fits) -- the caller issues the layers one by one.
extern "C" int geom_deform_chain_fwd_f32(int count, const geom_deform_fwd *layers, int *done, void *stream)
{
    if (count <= 0 || count > GEOM_DEFORM_CHAIN_MAX || !layers || !done || ((uintptr_t)done & 127)) return GEOM_EINVAL;
    DbFwdChain c{};
    for (int l = 0; l < count; ++l) {
        geom_deform_fwd a = layers[l];
        int code = db_check_shape(a.b, a.nv, a.c, a.k, a.ell_w);
        if (code) return code;
        if (a.b != layers[0].b || a.nv != layers[0].nv || a.ell_col != layers[0].ell_col || a.ell_val != layers[0].ell_val ||
            a.tail_col != layers[0].tail_col || a.tail_val != layers[0].tail_val)
            return GEOM_EINVAL;
        if (!a.w_next && l + 1 < count) return GEOM_EINVAL;                          // only the last layer may lack a product
        if (l > 0 && a.s_in != layers[l - 1].s_out) return GEOM_EINVAL;              // a chain
        if (l > 1 && a.s_out && a.s_out == layers[l - 1].s_out) return GEOM_EINVAL; // (ping-pong at least)
        if ((code = db_check_fwd(a))) return code;
        c.layer[l] = a;
    }
    if (layers[0].b == 0 || layers[0].nv == 0) return 0;
    if (!geom_deform_chain_fits(layers[0].nv)) return GEOM_EUNSUPPORTED;
    c.count = count, c.done = done;
    hipLaunchKernelGGL(db_fwd_chain_kernel, dim3(8 * c.layer[0].vpx), dim3(DB_THREADS), 0, static_cast<hipStream_t>(stream), c);
    return geom::launch_status();
}
