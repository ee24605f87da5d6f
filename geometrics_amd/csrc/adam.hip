// Multi-tensor Adam for the replicated 0N-GCN parameters (the optimiser the reference drivers use:
// GEOMetrics.py:73, optim.Adam(lr=1e-4)).  ONE launch for up to GEOM_ADAM_MAX_TENSORS parameter tensors; the step
// counter and the running beta powers live in device memory, so the update is HIP-graph replayable with no host
// scalars baked in.
//
// Who advances the step state?  Every workgroup reads {t, b1^t, b2^t} at its start and derives the bias corrections
// of step t+1 from it; the state may only change after the LAST workgroup has read it.  Round 1 used a 1-thread tick
// kernel in front (a 4.6 us launch floor per step); a single last-arriver counter was measured and rejected (6144
// same-address atomics serialise to ~50 us).  Here arrivals go through a two-level tree: workgroup w arrives at
// leaf counter w % 64, the last arriver of a leaf arrives at the root, the last arriver of the root writes the new
// state and re-arms the counters -- at most ceil(N/64) + 64 same-address atomics on any word (~1 us for the bench's
// 254 workgroups), all off the critical path except the final hop.  `advance` = 0 skips the protocol: that is how an
// optimiser with more than 64 tensors issues several launches that all use the bias corrections of ONE step (only
// the last launch advances).
//
// geom_adam_table_step_f32: the same step as ONE launch for ANY number of tensors.  The per-tensor records no longer travel
// as a by-value kernel argument (64 tensors fill it) but live in a caller-allocated DEVICE table, and the learning rate is read
// from a device array lr[group] -- a replayed HIP graph follows a changed lr without a re-capture.  Layout: structure of
// arrays, 48 * count bytes (geom_adam_table_bytes): p[count], g[count], m[count], v[count] (device pointers), n[count]
// (int64), then first_block[count] and group[count] (int32); workgroups [first_block[i], first_block[i + 1]) own tensor i.
// Chosen over a per-workgroup tensor map (one int per workgroup): both cost TWO dependent memory round trips per workgroup
// (the map / the prefix array, then the record), but the map is 4 bytes per workgroup -- 2 MB for the driver's 520 000
// workgroups, rebuilt and uploaded whenever a pointer moves -- where this table is 48 bytes per tensor.  The prefix array is
// not walked by a binary search (1 + log2(count) DEPENDENT loads: 9 round trips at 168 tensors) but counted: the 256 threads
// load first_block[] side by side (independent loads, one round trip, ceil(count / 256) per thread) and the number of entries
// <= blockIdx.x, summed over the wave ballots and the four waves (LDS, published by the barrier the state read has anyway), is
// the tensor's index + 1.  (The state read every workgroup has anyway sits between the two; the compiler does not overlap it
// with the count.)  Arithmetic, step state, arrival tree and the float4 / scalar-tail element path are the ones of
// adam_kernel: same bits.  The lookup is uniform per workgroup and uses plain loads; every value written to memory goes
// through the vector stores of adam_elements / the atomics of adam_math.h.
// Resources (tools/kernel_resources.sh, gfx950): adam_kernel 46 VGPR / 34 SGPR / 12 bytes of LDS, adam_table_kernel 46 VGPR /
// 33 SGPR / 28 bytes of LDS; both 0 bytes of scratch, no spills, 8 waves per SIMD.
// Update rule = torch.optim.Adam (no weight decay, no amsgrad):
//   m = b1*m + (1-b1)*g ; v = b2*v + (1-b2)*g*g
//   p -= lr / (1-b1^t) * m / (sqrt(v) / sqrt(1-b2^t) + eps)
#include "geom_common.h"
#include "adam_math.h"

namespace {

using geom::adam_update;

struct AdamTensors {
    float *p[GEOM_ADAM_MAX_TENSORS];
    const float *g[GEOM_ADAM_MAX_TENSORS];
    float *m[GEOM_ADAM_MAX_TENSORS];
    float *v[GEOM_ADAM_MAX_TENSORS];
    int64_t n[GEOM_ADAM_MAX_TENSORS];
    int first_block[GEOM_ADAM_MAX_TENSORS + 1]; // workgroups [first_block[i], first_block[i+1]) own tensor i
    int count;
};

// the 1024 elements [1024 * local, 1024 * local + 1024) of one tensor: a float4 per thread where all four pointers are 16-byte
// aligned and the four elements exist, else element by element
__device__ __forceinline__ void adam_elements(float *p, const float *g, float *m, float *v, int64_t n, int local, float b1,
                                              float b2, float eps, float grad_scale, const geom::AdamStep &as)
{
    const float step_size = as.step_size, bc2_sqrt = as.bc2_sqrt;
    const int64_t base = ((int64_t)local * 256 + threadIdx.x) * 4;
    const bool vec = ((((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15) == 0);
    if (base + 4 <= n && vec) {
        float4 pp = *reinterpret_cast<float4 *>(p + base);
        const float4 gg = *reinterpret_cast<const float4 *>(g + base);
        float4 mm = *reinterpret_cast<float4 *>(m + base);
        float4 vv = *reinterpret_cast<float4 *>(v + base);
        adam_update(pp.x, gg.x, mm.x, vv.x, b1, b2, eps, grad_scale, step_size, bc2_sqrt);
        adam_update(pp.y, gg.y, mm.y, vv.y, b1, b2, eps, grad_scale, step_size, bc2_sqrt);
        adam_update(pp.z, gg.z, mm.z, vv.z, b1, b2, eps, grad_scale, step_size, bc2_sqrt);
        adam_update(pp.w, gg.w, mm.w, vv.w, b1, b2, eps, grad_scale, step_size, bc2_sqrt);
        *reinterpret_cast<float4 *>(m + base) = mm;
        *reinterpret_cast<float4 *>(v + base) = vv;
        *reinterpret_cast<float4 *>(p + base) = pp;
    } else {
        for (int64_t i = base; i < n && i < base + 4; ++i) {
            float pi = p[i], mi = m[i], vi = v[i];
            adam_update(pi, g[i], mi, vi, b1, b2, eps, grad_scale, step_size, bc2_sqrt);
            m[i] = mi;
            v[i] = vi;
            p[i] = pi;
        }
    }
}

// state: [0] t (float), [1] b1^t, [2] b2^t, [3] root arrivals, [4..67] leaf arrivals (uint words)
__global__ __launch_bounds__(256) void adam_kernel(AdamTensors t, float lr, float b1, float b2, float eps,
                                                   float grad_scale, float *state, int advance)
{
    // the tensor this workgroup works on: the last i with first_block[i] <= blockIdx.x (uniform binary search, <= 6 steps;
    // empty tensors own no workgroup and are skipped by it)
    int lo = 0, hi = t.count - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if ((int)blockIdx.x >= t.first_block[mid]) lo = mid;
        else hi = mid - 1;
    }
    const int which = lo;
    const int local = blockIdx.x - t.first_block[which];

    __shared__ float st[3];
    const geom::AdamStep as = geom::adam_read_state(state, st, lr, b1, b2);   // see adam_math.h for the ordering argument
    adam_elements(t.p[which], t.g[which], t.m[which], t.v[which], t.n[which], local, b1, b2, eps, grad_scale, as);

    if (!advance) return;
    geom::adam_arrive(state, as, blockIdx.x, gridDim.x);
}

// the layout of the device table (see the file header); one definition for the kernel and the size query
constexpr int TABLE_WORDS = 6; // 8-byte words per tensor: p, g, m, v, n, {first_block, group}

__global__ __launch_bounds__(256) void adam_table_kernel(const int64_t *table, int count, const float *lr, float b1, float b2,
                                                         float eps, float grad_scale, float *state, int advance)
{
    const int *first_block = reinterpret_cast<const int *>(table + 5 * (int64_t)count);
    const int *group = first_block + count;
    // the tensor this workgroup works on: (number of i with first_block[i] <= blockIdx.x) - 1.  first_block[] ascends and
    // first_block[0] = 0, so that is the last such i; empty tensors share their first workgroup with the next tensor and are
    // skipped.  Uniform trip count: every lane takes part in every ballot.
    __shared__ int below[4];
    __shared__ float st[3];
    int mine = 0;
    for (int i0 = 0; i0 < count; i0 += 256) {
        const int i = i0 + (int)threadIdx.x;
        const bool le = i < count && first_block[i] <= (int)blockIdx.x;
        mine += __popcll(__ballot(le));
    }
    if ((threadIdx.x & (GEOM_WAVE - 1)) == 0) below[threadIdx.x / GEOM_WAVE] = mine;
    geom::adam_read_state(state, st, 0.f, b1, b2); // its barrier publishes below[] too; lr is not known yet
    int which = below[0] + below[1] + below[2] + below[3] - 1; // uniform
    if (which < 0) which = 0;                                  // a table whose first_block[0] is not 0: stay inside it
    const int local = (int)blockIdx.x - first_block[which];
    const geom::AdamStep as = geom::adam_step_from(st, lr[group[which]], b1, b2);

    float *p = reinterpret_cast<float *>(table[which]);
    const float *g = reinterpret_cast<const float *>(table[count + which]);
    float *m = reinterpret_cast<float *>(table[2 * (int64_t)count + which]);
    float *v = reinterpret_cast<float *>(table[3 * (int64_t)count + which]);
    adam_elements(p, g, m, v, table[4 * (int64_t)count + which], local, b1, b2, eps, grad_scale, as);

    if (!advance) return;
    geom::adam_arrive(state, as, blockIdx.x, gridDim.x);
}

} // namespace

extern "C" int geom_adam_step_f32(int count, float *const *params, const float *const *grads, float *const *exp_avg,
                                  float *const *exp_avg_sq, const int64_t *sizes, float lr, float beta1, float beta2,
                                  float eps, float grad_scale, float *state, int advance, void *stream)
{
    if (count < 0 || count > GEOM_ADAM_MAX_TENSORS) return GEOM_ETOOBIG;
    if (count == 0) return 0;
    if (!params || !grads || !exp_avg || !exp_avg_sq || !sizes || !state) return GEOM_EINVAL;
    AdamTensors t;
    int64_t blocks = 0;
    for (int i = 0; i < count; ++i) {
        if (!params[i] || !grads[i] || !exp_avg[i] || !exp_avg_sq[i] || sizes[i] < 0) return GEOM_EINVAL;
        t.p[i] = params[i];
        t.g[i] = grads[i];
        t.m[i] = exp_avg[i];
        t.v[i] = exp_avg_sq[i];
        t.n[i] = sizes[i];
        t.first_block[i] = (int)blocks;
        blocks += (sizes[i] + 1023) / 1024; // 256 threads x 4 elements
        if (blocks > 0x3fffffff) return GEOM_ETOOBIG;
    }
    t.first_block[count] = (int)blocks;
    t.count = count;
    if (blocks == 0) blocks = 1; // only empty tensors: one workgroup still advances the state
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(adam_kernel, dim3((unsigned)blocks), dim3(256), 0, s, t, lr, beta1, beta2, eps, grad_scale, state,
                       advance);
    return geom::launch_status();
}

extern "C" int64_t geom_adam_table_bytes(int count, int64_t total_blocks)
{
    if (count < 0 || total_blocks < 0) return GEOM_EINVAL;
    if (total_blocks > 0x3fffffff) return GEOM_ETOOBIG;
    return (int64_t)count * TABLE_WORDS * 8;
}

extern "C" int geom_adam_table_step_f32(int count, const void *table, int64_t total_blocks, const float *lr, float beta1,
                                        float beta2, float eps, float grad_scale, float *state, int advance, void *stream)
{
    if (count < 0 || total_blocks < 0) return GEOM_EINVAL;
    if (count == 0) return 0;
    if (!table || !lr || !state || ((uintptr_t)table & 7)) return GEOM_EINVAL;
    if (total_blocks > 0x3fffffff) return GEOM_ETOOBIG;
    if (total_blocks == 0) total_blocks = 1; // only empty tensors: one workgroup still advances the state
    hipLaunchKernelGGL(adam_table_kernel, dim3((unsigned)total_blocks), dim3(256), 0, static_cast<hipStream_t>(stream),
                       static_cast<const int64_t *>(table), count, lr, beta1, beta2, eps, grad_scale, state, advance);
    return geom::launch_status();
}
