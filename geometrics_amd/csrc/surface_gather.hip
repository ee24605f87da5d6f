// Backward of the sampled-surface losses (batch_point_to_point / batch_point_to_surface, reference utils.py:393-502
// under autograd) as a GATHER: every vertex sums the contributions of the sampled points and gt points that landed on
// its incident faces, in a fixed order.
//
// The scatter formulation (sample_loss.hip: one thread per point, nine fp32 atomics into a zeroed grad_verts) costs
// 26 us for 432 000 atomics at the BASELINE shard, needs a zero-fill, and adds in arrival order, so the last bits of
// the gradient change from run to run.  Here the points are counting-sorted by face, in two launches:
//   finalize  (forward side, behind the two scans; geom_surface_finalize_w_f32, or the role workgroups of the fused scan
//             launch in tri_distance.hip -- the same body, finalize_body.h) one workgroup per mesh, everything in LDS: every
//             point's gradient record -- (point - partner) * coefficient and its three corner weights, two float4 -- unless
//             the scans wrote it already; the points counted into their faces, an exclusive scan of the counts -> offsets,
//             and every face's segment put in ASCENDING ID ORDER (arrival order is not reproducible, id order is) by ranking
//             every id against its segment.  Any distribution is handled exactly -- 1.2 points per face on the 5120-face
//             BASELINE mesh, 6 on average and dozens on the large faces of the reference's 960-face training template.
//             One more workgroup reduces the two loss sums (fixed tree).
//   gather    (the whole backward; geom_surface_gather_w_f32) eight lanes per (mesh, vertex), one incident (face, corner)
//             each from a static CSR built once per face list: walk the face's segment, eight records in flight,
//             accumulate with this corner's barycentric weight; the lanes' partial sums are folded in lane order.
// grad_verts is written once per element (no zero-fill, no float atomics) and is bit-reproducible.  The scratch the two
// launches share is laid out in surface_layout.h.
#include "geom_common.h"
#include "device_facts.h"
#include "tri_math.h"
#include "surface_layout.h"
#include "finalize_body.h"

namespace {

using geom::V3;

constexpr int SGA_THREADS = 256;
constexpr int ORD_THREADS = 1024;
constexpr int ORD_WAVES = ORD_THREADS / GEOM_WAVE;
constexpr int VTX_LANES = 8;    // lanes that share a vertex in the gather: one incident face each, then an ordered fold
// dynamic LDS one workgroup may take for the ordering pass: what the device grants (160 KiB on gfx950; 64 KiB assumed of an
// unknown one) minus 10 KiB for the kernels' static arrays, so a part with less LDS answers GEOM_EUNSUPPORTED instead of
// failing the launch
inline size_t ord_lds_limit(const geom::DeviceFacts *dev)
{
    const size_t have = dev ? dev->lds_per_block_optin : 64 * 1024;
    const size_t limit = have > 16 * 1024 ? have - 10 * 1024 : have;
    return limit > 150 * 1024 ? 150 * 1024 : limit;
}

using geom_finalize::OTHER_NONE;
using geom_finalize::OTHER_NN;
using geom_finalize::OTHER_TRI;
using geom_finalize::FinalizeArgs;

// gradient contribution of a point to corner c of its face, from its two records
__device__ __forceinline__ V3 apply_record(float4 g, float4 w, int c)
{
    const float wc = c == 0 ? w.x : (c == 1 ? w.y : w.z);
    if (g.w != 0.f && wc == 0.f) return geom::mk(0.f, 0.f, 0.f);
    return geom::mk(g.x, g.y, g.z) * wc;
}

// the n points of a face (seg[s0 ...], in stored order) added to corner c's sum: eight records in flight
__device__ __forceinline__ V3 walk_segment(const int *seg, const float4 *rec, int s0, int n, int c, V3 acc)
{
    for (int h = 0; h < n; h += 8) {
        int id[8];
        float4 g[8], w[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) id[k] = h + k < n ? seg[s0 + h + k] : 0;
#pragma unroll
        for (int k = 0; k < 8; ++k)
            if (h + k < n) g[k] = rec[2 * id[k]], w[k] = rec[2 * id[k] + 1];
#pragma unroll
        for (int k = 0; k < 8; ++k)
            if (h + k < n) acc = acc + apply_record(g[k], w[k], c);
    }
    return acc;
}

// ---------------------------------------------------------------------------------------------------------------
// Forward-side FINALIZE: one launch after the two scans that (a) reduces the loss, (b) prepares the backward.
//
// One workgroup per mesh (1024 threads), everything that is shared in LDS:
//   * every thread takes its points (ids tid, tid + 1024, ...), forms their gradient records -- (point - partner) *
//     coefficient and the three corner weights, two float4 per point -- and counts them into their face with an LDS
//     atomic, remembering the arrival slot;
//   * exclusive scan of the face counts -> offsets; ids dropped at offset + slot; every id is then ranked against its
//     face's segment (LDS, independent loads) and written to its ASCENDING place: the order the gather adds in is a
//     function of the data only, never of timing;
//   * one more workgroup reduces the two loss sums (fixed tree) meanwhile.
// The backward is then ONE launch (surface_vertex_gather_kernel) and no global atomic.
template <bool REGS>
__global__ __launch_bounds__(ORD_THREADS) void surface_finalize_kernel(FinalizeArgs a)
{
    extern __shared__ __attribute__((aligned(16))) int ord_lds[];
    geom_finalize::surface_finalize_body<REGS, ORD_THREADS>(a, ord_lds, blockIdx.x);
}

struct VGatherArgs {
    const int *vf_ptr, *vf_item;
    const int *off, *seg;
    const float4 *rec;
    const float *grad; // upstream gradient of the loss (device scalar), may be null (= 1)
    float *grad_verts;
    int nv, nf, per;
    const int *status; // [b + 1] (surface_layout.h)
    int b;
    const float *mesh_weight; // [b] or null: mesh m's gradient times w[m] (the loss was formed with the same weights)
};

// The backward: eight lanes per (mesh, vertex), one incident (face, corner) each; a face's segment is walked in its
// stored (ascending id) order, eight records in flight; lanes folded in lane order; result scaled by 2 * upstream.
__global__ __launch_bounds__(SGA_THREADS) void surface_vertex_gather_kernel(VGatherArgs a)
{
    const int t = blockIdx.x * SGA_THREADS + threadIdx.x;
    const int vtx = t / VTX_LANES, j = t % VTX_LANES;
    const int mesh = blockIdx.y;
    const bool live = vtx < a.nv;
    V3 acc = geom::mk(0.f, 0.f, 0.f);
    // a mesh whose ordering (or the loss it belongs to) was given up by a finalize role of the scan launch: NaN, loudly --
    // never a walk through a half-built order
    const bool broken = a.status[mesh] != 0 || a.status[a.b] != 0;
    if (live && !broken) {
        const int *off = a.off + (int64_t)mesh * (a.nf + 1);
        const int *seg = a.seg + (int64_t)mesh * a.per;
        const float4 *rec = a.rec + 2 * (int64_t)mesh * a.per;
        const int e1 = a.vf_ptr[vtx + 1];
        for (int e = a.vf_ptr[vtx] + j; e < e1; e += VTX_LANES) {
            const int item = a.vf_item[e];
            const int f = item >> 2, c = item & 3;
            const int s0 = off[f], n = off[f + 1] - s0;
            acc = walk_segment(seg, rec, s0, n, c, acc);
        }
    }
    V3 total = acc;
#pragma unroll
    for (int k = 1; k < VTX_LANES; ++k) {
        const V3 other = geom::mk(__shfl_down(acc.x, k, VTX_LANES), __shfl_down(acc.y, k, VTX_LANES),
                                  __shfl_down(acc.z, k, VTX_LANES));
        total = total + other;
    }
    if (live && j == 0) {
        float s = broken ? __builtin_nanf("") : 2.f * (a.grad ? a.grad[0] : 1.f);
        if (a.mesh_weight) s *= a.mesh_weight[mesh];
        float *G = a.grad_verts + ((int64_t)mesh * a.nv + vtx) * 3;
        G[0] = total.x * s;
        G[1] = total.y * s;
        G[2] = total.z * s;
    }
}

inline size_t order_lds_bytes(int nf, int per) { return ((size_t)nf + 1 + per + ORD_WAVES + 4) * sizeof(int); }

// ---------------------------------------------------------------------------------------------------------------
// The same two launches for a RAGGED batch: b meshes that own their faces inside one union (ragged.group_faces).
//
// finalize: the body above once more (finalize_body.h: FinalizeRagged), one workgroup per mesh; mesh m's face count is read
// from face_off on the device, a point's bin is the position of its union face id inside the mesh (face_pos, the inverse of
// face_list: no search), and what leaves the workgroup is one (start in seg, count) pair per UNION face.  a.nf arrives as the
// face count the dynamic LDS was sized for; a mesh with more faces cannot be ordered: its workgroup marks its status word and
// gives every face of the mesh a negative count, which the gather turns into NaN.  Nothing else of that mesh is touched.
template <bool REGS>
__global__ __launch_bounds__(ORD_THREADS) void surface_finalize_ragged_kernel(FinalizeArgs a, geom_finalize::FinalizeRagged fc)
{
    extern __shared__ __attribute__((aligned(16))) int ord_lds[];
    const int mesh = blockIdx.x;
    if (mesh < a.b) { // (block b: the loss role)
        // both inside [0, nft] whatever face_off holds
        fc.face0 = min(max(fc.face_off[mesh], 0), fc.nft);
        const int nf = min(max(fc.face_off[mesh + 1] - fc.face0, 0), fc.nft - fc.face0);
        if (nf > a.nf) {
            for (int k = threadIdx.x; k < nf; k += ORD_THREADS) {
                const int face = fc.face_list[fc.face0 + k];
                if ((unsigned)face < (unsigned)fc.nft) fc.pair[face] = make_int2(0, -1), fc.fmesh[face] = mesh;
            }
            if (threadIdx.x == 0) a.status[mesh] = 1;
            return;
        }
        a.nf = nf;
    }
    geom_finalize::surface_finalize_body<REGS, ORD_THREADS, geom_finalize::FinalizeNoWait, geom_finalize::FIN_REG_POINTS / ORD_THREADS,
                                         false, geom_finalize::FinalizeRagged>(a, ord_lds, blockIdx.x, geom_finalize::FinalizeNoWait(), fc);
}

struct RaggedGatherArgs {
    const int *vf_ptr, *vf_item;
    const int2 *pair;
    const int *fmesh, *seg;
    const float4 *rec;
    const float *grad; // upstream gradient of the loss (device scalar), may be null (= 1)
    float *grad_verts;
    int nv;
    const float *mesh_weight; // [b] or null
};

// gather: surface_vertex_gather_kernel's walk over the UNION's vertices -- eight lanes per vertex, entries j, j + 8, ... of the
// union's vertex-to-face table, every face's segment entered through its pair, lanes folded in lane order, every element of
// grad_verts [nv,3] written once.  A vertex's factor is the weight of the mesh of its incident faces; a vertex whose faces
// belong to different meshes (no disjoint union) has none: NaN when weights are given.  A face whose mesh was not ordered
// (count < 0) makes its vertices NaN.
__global__ __launch_bounds__(SGA_THREADS) void surface_vertex_gather_ragged_kernel(RaggedGatherArgs a)
{
    const int t = blockIdx.x * SGA_THREADS + threadIdx.x;
    const int vtx = t / VTX_LANES, j = t % VTX_LANES;
    const bool live = vtx < a.nv;
    V3 acc = geom::mk(0.f, 0.f, 0.f);
    int broken = 0, mesh = -1; // mesh: -1 none yet, -2 more than one
    if (live) {
        const int e1 = a.vf_ptr[vtx + 1];
        for (int e = a.vf_ptr[vtx] + j; e < e1; e += VTX_LANES) {
            const int item = a.vf_item[e];
            const int f = item >> 2, c = item & 3;
            const int2 p = a.pair[f];
            if (a.mesh_weight) {
                const int m = a.fmesh[f];
                if (m >= 0) mesh = mesh == -1 || mesh == m ? m : -2;
            }
            broken |= p.y < 0;
            acc = walk_segment(a.seg, a.rec, p.x, p.y, c, acc);
        }
    }
    V3 total = acc;
#pragma unroll
    for (int k = 1; k < VTX_LANES; ++k) {
        const V3 other = geom::mk(__shfl_down(acc.x, k, VTX_LANES), __shfl_down(acc.y, k, VTX_LANES),
                                  __shfl_down(acc.z, k, VTX_LANES));
        total = total + other;
    }
    int any_broken = broken, vmesh = mesh;
#pragma unroll
    for (int k = 1; k < VTX_LANES; ++k) {
        any_broken |= __shfl_down(broken, k, VTX_LANES);
        const int m = __shfl_down(mesh, k, VTX_LANES);
        if (m != -1) vmesh = vmesh == -1 || vmesh == m ? m : -2;
    }
    if (live && j == 0) {
        float s = any_broken || vmesh == -2 ? __builtin_nanf("") : 2.f * (a.grad ? a.grad[0] : 1.f);
        if (a.mesh_weight && vmesh >= 0) s *= a.mesh_weight[vmesh];
        float *G = a.grad_verts + (int64_t)vtx * 3;
        G[0] = total.x * s;
        G[1] = total.y * s;
        G[2] = total.z * s;
    }
}

// faces per mesh the ragged finalize launch can order beside `per` points (what its LDS holds), < 0: not even the points fit
inline int64_t ragged_face_fit(int64_t per, const geom::DeviceFacts *dev)
{
    return (int64_t)(ord_lds_limit(dev) / sizeof(int)) - 1 - per - ORD_WAVES - 4;
}

} // namespace
// int32 words of the scratch (surface_layout.h) for a batch of b meshes of nf faces, cap = num + n_gt points each
extern "C" int64_t geom_surface_order_words(int b, int nf, int num, int n_gt)
{
    if (b <= 0 || nf < 0 || num < 0 || n_gt < 0) return 0;
    const int64_t cap = (int64_t)num + n_gt;
    return geom_surface_status_offset(b, nf, cap) + geom_surface_status_ints(b);
}

// mesh_weight (may be NULL = all ones): [b] device floats; the loss becomes sum_m w[m] * (mesh m's two sums) -- several
// equal-size batches (the stages of a cascade) stacked into ONE call, each with its own factor.  The gradient records do not
// carry the weights: geom_surface_gather_w_f32 applies the same array.
extern "C" int geom_surface_finalize_w_f32(int b, int nf, int num, const int64_t *choices, const float *u, const float *v,
                                           const float *points, int n_gt, const float *gt, const int *idx_g,
                                           const int *idx_p, const int *index, const float *closest, const float *weights,
                                           const float *sq_sample, const float *sq_other, float scale_sample,
                                           float scale_other, float coef_sample, float coef_other, int want_order,
                                           int records_ready, int *order, float *loss, const float *mesh_weight, void *stream)
{
    if (b < 0 || nf < 0 || num < 0 || n_gt < 0) return GEOM_EINVAL;
    if (!loss || !order || ((uintptr_t)order & 15)) return GEOM_EINVAL;
    if (b == 0) return 0;
    if ((num > 0 && !sq_sample) || (n_gt > 0 && !sq_other)) return GEOM_EINVAL;
    if (idx_p && index) return GEOM_EINVAL;
    if (b > 65535) return GEOM_ETOOBIG;
    const int other = idx_p ? OTHER_NN : (index ? OTHER_TRI : OTHER_NONE);
    const int64_t per64 = (int64_t)num + (other != OTHER_NONE ? n_gt : 0);
    if (per64 > 0x3fffffff) return GEOM_ETOOBIG;
    const int per = (int)per64;
    const geom::DeviceFacts *dev = geom::device_facts();
    const size_t ord_lds = ord_lds_limit(dev);
    if (want_order) {
        if (num > 0 && (!choices || !u || !v || !points || !gt || !idx_g || n_gt == 0)) return GEOM_EINVAL;
        if (index && (!closest || !weights || !gt)) return GEOM_EINVAL;
        if (order_lds_bytes(nf, per) > ord_lds) return GEOM_EUNSUPPORTED;
    }
    const SurfaceScratch scr = geom_surface_scratch(order, b, nf, (int64_t)num + n_gt);
    FinalizeArgs a{choices, u, v, points, gt, idx_g, idx_p, index, closest, weights, sq_sample, sq_other, scale_sample,
                   scale_other, coef_sample, coef_other, b, nf, num, n_gt, other, per, want_order ? 1 : 0, records_ready ? 1 : 0, scr.off,
                   scr.seg, scr.pface, scr.slot, scr.rec, loss, scr.status, mesh_weight};
    hipStream_t s = static_cast<hipStream_t>(stream);
    // without ordering the single (loss) workgroup touches only its reduction scratch: independent of nf, so the
    // documented fallback beyond the ordering limit (want_order = 0 + scatter backward) really launches
    const size_t lds = geom_finalize::finalize_lds_ints(nf, per, ORD_THREADS, want_order != 0) * sizeof(int);
    if (per <= geom_finalize::FIN_REG_POINTS) {
        (void)geom::allow_dynamic_lds(surface_finalize_kernel<true>, (int)ord_lds + 1024, dev); // (a refusal: the launch reports it)
        hipLaunchKernelGGL(surface_finalize_kernel<true>, dim3(want_order ? b + 1 : 1), dim3(ORD_THREADS), lds, s, a);
    } else {
        (void)geom::allow_dynamic_lds(surface_finalize_kernel<false>, (int)ord_lds + 1024, dev);
        hipLaunchKernelGGL(surface_finalize_kernel<false>, dim3(want_order ? b + 1 : 1), dim3(ORD_THREADS), lds, s, a);
    }
    return geom::launch_status();
}

extern "C" int geom_surface_finalize_f32(int b, int nf, int num, const int64_t *choices, const float *u, const float *v,
                                         const float *points, int n_gt, const float *gt, const int *idx_g,
                                         const int *idx_p, const int *index, const float *closest, const float *weights,
                                         const float *sq_sample, const float *sq_other, float scale_sample,
                                         float scale_other, float coef_sample, float coef_other, int want_order,
                                         int records_ready, int *order, float *loss, void *stream)
{
    return geom_surface_finalize_w_f32(b, nf, num, choices, u, v, points, n_gt, gt, idx_g, idx_p, index, closest, weights, sq_sample,
                                       sq_other, scale_sample, scale_other, coef_sample, coef_other, want_order, records_ready, order,
                                       loss, nullptr, stream);
}

// mesh_weight (may be NULL): the per-mesh factors of geom_surface_finalize_w_f32; mesh m's gradient = w[m] * 2 * grad[0] * (...)
extern "C" int geom_surface_gather_w_f32(int b, int nv, int nf, const int *vf_ptr, const int *vf_item, int num, int n_gt,
                                         int has_other, const int *order, const float *grad, const float *mesh_weight,
                                         float *grad_verts, void *stream)
{
    if (b < 0 || nv < 0 || nf < 0 || num < 0 || n_gt < 0) return GEOM_EINVAL;
    if (b == 0 || nv == 0) return 0;
    if (!vf_ptr || !vf_item || !order || !grad_verts || ((uintptr_t)order & 15)) return GEOM_EINVAL;
    if (b > 65535) return GEOM_ETOOBIG;
    const int per = num + (has_other ? n_gt : 0);
    const SurfaceScratch scr = geom_surface_scratch(const_cast<int *>(order), b, nf, (int64_t)num + n_gt); // (read only here)
    VGatherArgs a{vf_ptr, vf_item, scr.off, scr.seg, scr.rec, grad, grad_verts, nv, nf, per, scr.status, b, mesh_weight};
    hipLaunchKernelGGL(surface_vertex_gather_kernel, dim3(((int64_t)nv * VTX_LANES + SGA_THREADS - 1) / SGA_THREADS, b),
                       dim3(SGA_THREADS), 0, static_cast<hipStream_t>(stream), a);
    return geom::launch_status();
}

extern "C" int geom_surface_gather_f32(int b, int nv, int nf, const int *vf_ptr, const int *vf_item, int num, int n_gt,
                                       int has_other, const int *order, const float *grad, float *grad_verts, void *stream)
{
    return geom_surface_gather_w_f32(b, nv, nf, vf_ptr, vf_item, num, n_gt, has_other, order, grad, nullptr, grad_verts, stream);
}

// ---- ragged batches (surface_layout.h: RaggedSurfaceScratch) ----
extern "C" int64_t geom_surface_order_ragged_words(int b, int nft, int num, int n_gt)
{
    if (b <= 0 || nft < 0 || num < 0 || n_gt < 0) return 0;
    return geom_surface_ragged_status_offset(b, nft, (int64_t)num + n_gt) + geom_surface_status_ints(b);
}

extern "C" int geom_surface_ragged_face_cap(int nft, int num, int n_gt)
{
    if (nft < 0 || num < 0 || n_gt < 0) return GEOM_EINVAL;
    const int64_t fit = ragged_face_fit((int64_t)num + n_gt, geom::device_facts());
    return fit < 0 ? GEOM_EUNSUPPORTED : (int)(fit < nft ? fit : nft);
}

extern "C" int geom_surface_finalize_ragged_f32(int b, int nft, const int *face_list, const int *face_off, const int *face_pos,
                                                int num, const int64_t *choices, const float *u, const float *v,
                                                const float *points, int n_gt, const float *gt, const int *idx_g,
                                                const int *idx_p, const int *index, const float *closest,
                                                const float *weights, const float *sq_sample, const float *sq_other,
                                                float scale_sample, float scale_other, float coef_sample, float coef_other,
                                                int *order, float *loss, const float *mesh_weight, void *stream)
{
    if (b < 0 || nft < 0 || num < 0 || n_gt < 0) return GEOM_EINVAL;
    if (!order || ((uintptr_t)order & 15)) return GEOM_EINVAL;
    if (b == 0) return 0;
    if (!face_off || (nft > 0 && (!face_list || !face_pos))) return GEOM_EINVAL;
    if (loss && ((num > 0 && !sq_sample) || (n_gt > 0 && !sq_other))) return GEOM_EINVAL;
    if (mesh_weight && !loss) return GEOM_EINVAL; // (the factors enter the loss here and the gradient in the gather)
    if (!idx_p == !index) return GEOM_EINVAL;     // one partner kind: the two-sided loss's or the one-sided loss's
    if (num > 0 && (!choices || !u || !v || !points || !gt || !idx_g || n_gt == 0)) return GEOM_EINVAL;
    if (index && (!closest || !weights || !gt)) return GEOM_EINVAL;
    if (b > 65535) return GEOM_ETOOBIG;
    const int64_t per64 = (int64_t)num + n_gt;
    if ((int64_t)b * per64 > 0x3fffffff) return GEOM_ETOOBIG; // (ids of the flat batch, doubled, index the records)
    const int per = (int)per64;
    const geom::DeviceFacts *dev = geom::device_facts();
    const int64_t fit = ragged_face_fit(per64, dev);
    if (fit < 0) return GEOM_EUNSUPPORTED;
    const int face_cap = (int)(fit < nft ? fit : nft);
    const RaggedSurfaceScratch scr = geom_surface_ragged_scratch(order, b, nft, per64);
    FinalizeArgs a{choices, u, v, points, gt, idx_g, idx_p, index, closest, weights, sq_sample, sq_other, scale_sample,
                   scale_other, coef_sample, coef_other, b, face_cap, num, n_gt, idx_p ? OTHER_NN : OTHER_TRI, per, 1, 0, nullptr,
                   scr.seg, scr.pface, scr.slot, scr.rec, loss, scr.status, mesh_weight};
    geom_finalize::FinalizeRagged fc{face_list, face_off, face_pos, scr.pair, scr.fmesh, nft, 0};
    hipStream_t s = static_cast<hipStream_t>(stream);
    const size_t ord_lds = ord_lds_limit(dev);
    const size_t lds = geom_finalize::finalize_lds_ints(face_cap, per, ORD_THREADS, true) * sizeof(int);
    if (per <= geom_finalize::FIN_REG_POINTS) {
        (void)geom::allow_dynamic_lds(surface_finalize_ragged_kernel<true>, (int)ord_lds + 1024, dev); // (a refusal: the launch reports it)
        hipLaunchKernelGGL(surface_finalize_ragged_kernel<true>, dim3(b + 1), dim3(ORD_THREADS), lds, s, a, fc);
    } else {
        (void)geom::allow_dynamic_lds(surface_finalize_ragged_kernel<false>, (int)ord_lds + 1024, dev);
        hipLaunchKernelGGL(surface_finalize_ragged_kernel<false>, dim3(b + 1), dim3(ORD_THREADS), lds, s, a, fc);
    }
    return geom::launch_status();
}

extern "C" int geom_surface_gather_ragged_f32(int b, int nv, int nft, const int *vf_ptr, const int *vf_item, int num, int n_gt,
                                              const int *order, const float *grad, const float *mesh_weight, float *grad_verts,
                                              void *stream)
{
    if (b < 0 || nv < 0 || nft < 0 || num < 0 || n_gt < 0) return GEOM_EINVAL;
    if (b == 0 || nv == 0) return 0;
    if (!vf_ptr || !vf_item || !order || !grad_verts || ((uintptr_t)order & 15)) return GEOM_EINVAL;
    if (b > 65535 || (int64_t)b * ((int64_t)num + n_gt) > 0x3fffffff) return GEOM_ETOOBIG;
    const RaggedSurfaceScratch scr = geom_surface_ragged_scratch(const_cast<int *>(order), b, nft, (int64_t)num + n_gt); // (read only here)
    RaggedGatherArgs a{vf_ptr, vf_item, scr.pair, scr.fmesh, scr.seg, scr.rec, grad, grad_verts, nv, mesh_weight};
    hipLaunchKernelGGL(surface_vertex_gather_ragged_kernel, dim3(((int64_t)nv * VTX_LANES + SGA_THREADS - 1) / SGA_THREADS),
                       dim3(SGA_THREADS), 0, static_cast<hipStream_t>(stream), a);
    return geom::launch_status();
}
