// Layout of the surface-loss backward scratch (`order`, int32 words) shared by the fused scan (which writes the
// gradient records) and the finalize / gather passes (csrc/surface_gather.hip):
//   off[b,nf+1] | seg[b,cap] | pface[b,cap] | slot[b,cap] | pad to 4 words | rec[b,cap,2] float4 | status[b+1, pad to 4]
// with cap = num + n_gt.  status[i] (i < b): 0 = mesh i's ordering is complete, anything else = the pass that orders it gave up
// (a finalize role of the scan launch whose wait timed out); status[b]: the same for the loss sum.  Written by EVERY finalize
// pass (0 on success), read by the gather backward: a mesh whose ordering is not there gets NaN gradients, never a walk
// through a half-built order.
#pragma once
#include <stdint.h>

static inline int64_t geom_surface_order_ints(int b, int nf, int64_t cap)
{
    return (((int64_t)b * (nf + 1) + 3 * (int64_t)b * cap) + 3) & ~3ll;
}
static inline int64_t geom_surface_status_ints(int b) { return ((int64_t)b + 1 + 3) & ~3ll; }
static inline int64_t geom_surface_status_offset(int b, int nf, int64_t cap) { return geom_surface_order_ints(b, nf, cap) + (int64_t)b * cap * 8; }

// The scratch carved up (float4: the including file has the HIP headers); a null `order` gives null members.
struct SurfaceScratch {
    int *off, *seg, *pface, *slot; // [b,nf+1], then [b,cap] each
    float4 *rec;                   // [b,cap,2]
    int *status;                   // [b+1]
};
static inline SurfaceScratch geom_surface_scratch(int *order, int b, int nf, int64_t cap)
{
    if (!order) return SurfaceScratch{};
    int *seg = order + (int64_t)b * (nf + 1), *pface = seg + (int64_t)b * cap;
    return SurfaceScratch{order, seg, pface, pface + (int64_t)b * cap, reinterpret_cast<float4 *>(order + geom_surface_order_ints(b, nf, cap)),
                          order + geom_surface_status_offset(b, nf, cap)};
}

// The same scratch for a RAGGED batch (b meshes that own their faces inside one union of nft faces):
//   pair[nft] (int2) | fmesh[nft] | seg[b,cap] | pface[b,cap] | slot[b,cap] | pad to 4 words | rec[b,cap,2] float4 | status[b+1, pad to 4]
// pair[f] = (where face f's points start in seg -- an index into the WHOLE seg array --, how many they are), written by the
// workgroup of the face's mesh; (0, 0) for a face of no mesh (written by the loss role's workgroup); count < 0: the mesh's
// ordering was given up (more faces than the launch's LDS holds; status[m] != 0 says the same per mesh).  fmesh[f]: the mesh that
// wrote the pair, -1 for none.  seg holds ids of the flat batch, m * cap + id, so rec is entered with them directly: the gather
// goes from a UNION face id to its records by pair[f] -> seg -> rec, the chain off[f], off[f+1] -> seg -> rec of the batched
// layout, and nothing has to be zeroed in front of the launch.
static inline int64_t geom_surface_ragged_order_ints(int b, int nft, int64_t cap)
{
    return ((3 * (int64_t)nft + 3 * (int64_t)b * cap) + 3) & ~3ll;
}
static inline int64_t geom_surface_ragged_status_offset(int b, int nft, int64_t cap)
{
    return geom_surface_ragged_order_ints(b, nft, cap) + (int64_t)b * cap * 8;
}
struct RaggedSurfaceScratch {
    int2 *pair;                // [nft]
    int *fmesh;                // [nft]
    int *seg, *pface, *slot;   // [b,cap] each
    float4 *rec;               // [b,cap,2]
    int *status;               // [b+1]
};
static inline RaggedSurfaceScratch geom_surface_ragged_scratch(int *order, int b, int nft, int64_t cap)
{
    if (!order) return RaggedSurfaceScratch{};
    int *fmesh = order + 2 * (int64_t)nft, *seg = fmesh + nft, *pface = seg + (int64_t)b * cap;
    return RaggedSurfaceScratch{reinterpret_cast<int2 *>(order), fmesh, seg, pface, pface + (int64_t)b * cap,
                                reinterpret_cast<float4 *>(order + geom_surface_ragged_order_ints(b, nft, cap)),
                                order + geom_surface_ragged_status_offset(b, nft, cap)};
}
