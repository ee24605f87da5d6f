// What every kernel file that talks to memory through buffer descriptors, or finishes a layer's activation, states the same
// way: the vector types of the builtins, the descriptor, the offset the hardware drops, 16-byte loads and stores, and the
// activation with its derivative.  Values only; nothing here holds state.
#pragma once
#include "geom_common.h"

namespace geom {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x3 __attribute__((ext_vector_type(3)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
struct __attribute__((packed, aligned(4))) f3u { float x, y, z; }; // three floats loaded as 12 bytes (4-byte aligned)

// Buffer addressing: a 32-bit byte offset per lane against a wave-uniform descriptor (half the address traffic of a flat
// access per instruction -- a VMEM instruction between two MFMAs costs its issue time), loads beyond the range return 0 and
// stores beyond it are dropped: predication without a branch in the MFMA stream.  An access that must not happen -- a row
// beyond the matrix, a column beyond the width, the group after the last -- gets the offset OOB instead of a branch around it.
// Besides the branches this keeps the memory counter countable: every load and store is issued on every path, so a wait for
// one of them is `all but the N youngest` with N known, and never drains the stores issued since.
constexpr unsigned OOB = 0x80000000u; // beyond every range: the hosts bound each array to < 2 GB
// a null pointer gives an empty range: every access of an absent optional operand is dropped
__device__ __forceinline__ __amdgpu_buffer_rsrc_t rsrc(const void *p, int64_t bytes)
{
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(p), 0, p ? (int)bytes : 0, 0x00020000);
}
// AGENT: an access that another workgroup of the SAME launch produces / consumes (sc1: through the XCD's L2 to the memory
// side, what an agent-scope atomic compiles to -- the eight L2s do not snoop each other)
constexpr int BUFFER_SC1 = 16;
template <bool AGENT = false>
__device__ __forceinline__ float4 ld4(__amdgpu_buffer_rsrc_t r, unsigned off)
{
    const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(r, off, 0, AGENT ? BUFFER_SC1 : 0);
    return make_float4(__uint_as_float(v.x), __uint_as_float(v.y), __uint_as_float(v.z), __uint_as_float(v.w));
}
template <bool AGENT = false>
__device__ __forceinline__ void st4(__amdgpu_buffer_rsrc_t r, unsigned off, float4 v)
{
    __builtin_amdgcn_raw_buffer_store_b128((u32x4){__float_as_uint(v.x), __float_as_uint(v.y), __float_as_uint(v.z), __float_as_uint(v.w)},
                                           r, off, 0, AGENT ? BUFFER_SC1 : 0);
}

// A layer's activation, and its derivative expressed through the saved OUTPUT (what torch's relu / elu backward use)
enum { ACT_NONE = 0, ACT_RELU = 1, ACT_ELU = 2 };
template <int ACT>
__device__ __forceinline__ float act_fwd(float v)
{
    if (ACT == ACT_RELU) return v <= 0.f ? 0.f : v; // (torch.relu: NaN stays NaN)
    if (ACT == ACT_ELU) return v > 0.f ? v : expm1f(v);
    return v;
}
template <int ACT>
__device__ __forceinline__ float act_bwd(float g, float out)
{
    if (ACT == ACT_RELU) return out <= 0.f ? 0.f : g; // (threshold_backward: a NaN output lets g through)
    if (ACT == ACT_ELU) return out > 0.f ? g : g * (out + 1.f); // (a NaN output: NaN)
    return g;
}

} // namespace geom
