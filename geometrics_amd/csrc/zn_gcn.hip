// 0N-GCN aggregation for gfx950: out = [ A . S[:, :k] | S[:, k:] ] + bias, activation fused.
//
// The reference multiplies by the DENSE row-normalised adjacency (layers.py:37, 111, 146:
// torch.mm/matmul(adj, support[..., :k]) -- V^2*k MACs and a V^2*4-byte read per layer with
// 99.7 % zeros at V=2562) and then torch.cat's the pass-through columns and adds the bias in
// two more passes.  Here one kernel reads `support` once and writes `out` once: a CSR row
// gather (6-7 neighbours on an icosphere, up to 33 on the reference's 482.obj poles) for
// the first k columns, a straight copy for the rest, bias and activation in the epilogue.
// The backward is the same kernel on CSR^T (the normalised adjacency is not symmetric) with
// the activation derivative folded into the read.
//
// One thread owns VEC consecutive columns of one row, so a wave reads/writes contiguous
// 256 B - 1 KiB runs; neighbour rows of the k-slice are re-read through L2 (the slice is
// b*V*k*4 bytes, 5.2 MB at the BASELINE shard).  HBM-bound: algorithmic bytes = read
// support + write out (+ CSR), see DESIGN.md.
//
// Three kernels -- zn_aggregate_kernel (CSR), zn_aggregate_ell_kernel (neighbour table, split 3 / 10) and
// zn_aggregate_ell_any_kernel (neighbour table, any width) -- share ONE statement of each step ("The aggregation
// kernels' shared steps"): Pack<VEC>'s element-wise operations; the neighbour term in two halves (term_load: the loads of
// one neighbour row, term_add: derivative + acc += w * v); the table-row load and its slots (load_table_row,
// load_table_slots, add_table_slots); the CSR run in batches (add_csr_run); the own element (own_element); the forward
// epilogue (Pack::bias_act); the straddling group's partial stores (Pack::store_below / store_from); the column-sum partials
// (write_colsum_partial) and their reduction (reduce_partials).  The summation rule -- table slots in slot order, then the
// tail in CSR order, un-fused, from 0.f, padded slots skipped -- is term_add under `if (the slot is in the row)` and nowhere
// else; the fused launches of zn_stack.hip, deform_block.hip and encoder_stack.hip are pinned to its bits.  The fast kernel
// keeps its own elements with the column sums over them and its tail's index prefetch as written (registers: DESIGN.md).
#include <type_traits>

#include "buffer_access.h"

namespace {

using namespace geom;

constexpr int GCN_THREADS = 256;

struct GcnArgs {
    const int *rowptr, *col;
    const float *val;
    const float *x;     // support (forward) or grad_out (backward)
    const float *bias;  // forward only, may be null
    const float *saved; // backward only: forward output, for the activation derivative
    float *y;
    int64_t rows;       // b * nv
    int nv, c, k;
};

// VEC consecutive floats of a row, moved as one float4 / float2 / float, with the element-wise steps of the kernels below.
template <int VEC>
struct PackVector;
template <>
struct PackVector<4> { using type = float4; };
template <>
struct PackVector<2> { using type = float2; };
template <>
struct PackVector<1> { using type = float; };

__device__ __forceinline__ float *elements(float4 &v) { return &v.x; }
__device__ __forceinline__ float *elements(float2 &v) { return &v.x; }
__device__ __forceinline__ float *elements(float &v) { return &v; }
__device__ __forceinline__ const float *elements(const float4 &v) { return &v.x; }
__device__ __forceinline__ const float *elements(const float2 &v) { return &v.x; }
__device__ __forceinline__ const float *elements(const float &v) { return &v; }

template <int VEC>
struct Pack {
    using Vector = typename PackVector<VEC>::type;
    Vector v;
    __device__ __forceinline__ void load(const float *p) { v = *reinterpret_cast<const Vector *>(p); }
    __device__ __forceinline__ void store(float *p) const { *reinterpret_cast<Vector *>(p) = v; }
    __device__ __forceinline__ float &at(int i) { return elements(v)[i]; }
    __device__ __forceinline__ float at(int i) const { return elements(v)[i]; }
    static __device__ __forceinline__ Pack zero()
    {
        Pack p;
#pragma unroll
        for (int i = 0; i < VEC; ++i) p.at(i) = 0.f;
        return p;
    }
    __device__ __forceinline__ void add(const Pack &o)
    {
#pragma unroll
        for (int i = 0; i < VEC; ++i) at(i) += o.at(i);
    }
    __device__ __forceinline__ void add_scaled(float w, const Pack &o) // += w * o: a product, then a sum (never fused)
    {
#pragma unroll
        for (int i = 0; i < VEC; ++i) at(i) += w * o.at(i);
    }
    template <int ACT>
    __device__ __forceinline__ void act_bwd_from(const Pack &out) // g -> g * act'(out)
    {
#pragma unroll
        for (int i = 0; i < VEC; ++i) at(i) = act_bwd<ACT>(at(i), out.at(i));
    }
    __device__ __forceinline__ void keep_where(unsigned bits) // element i stays where bit i is set (relu' from sign bits)
    {
#pragma unroll
        for (int i = 0; i < VEC; ++i) at(i) = (bits & (1u << i)) ? at(i) : 0.f;
    }
    // forward epilogue: + bias[col ...] (bias == null: none), activation.  WIDE: the bias is read as one vector (the fast kernel,
    // whose dispatcher checks its alignment), otherwise float by float
    template <int ACT, bool WIDE = false>
    __device__ __forceinline__ void bias_act(const float *bias, int col)
    {
        if (WIDE) {
            if (bias) {
                Pack b;
                b.load(bias + col);
                add(b);
            }
#pragma unroll
            for (int i = 0; i < VEC; ++i) at(i) = act_fwd<ACT>(at(i));
        } else {
#pragma unroll
            for (int i = 0; i < VEC; ++i) {
                float t = at(i);
                if (bias) t += bias[col + i];
                at(i) = act_fwd<ACT>(t);
            }
        }
    }
    __device__ __forceinline__ unsigned positive_bits() const // bit i = !(element i <= 0), the predicate relu' is defined by (act_bwd)
    {
        unsigned bits = 0u;
#pragma unroll
        for (int i = 0; i < VEC; ++i) bits |= at(i) <= 0.f ? 0u : 1u << i;
        return bits;
    }
    __device__ __forceinline__ void take_from(const Pack &o, int first) // elements first.. are o's
    {
#pragma unroll
        for (int i = 0; i < VEC; ++i)
            if (i >= first) at(i) = o.at(i);
    }
    // The pack holds columns c0 .. c0 + VEC - 1 of `row`.  Of the group that straddles column k, the aggregating thread stores
    // the columns below k and the pass-through thread those from k on, element by element; a whole group goes as one vector.
    __device__ __forceinline__ void store_below(float *row, int c0, int k) const
    {
        if (c0 + VEC <= k) {
            store(row + c0);
        } else {
#pragma unroll
            for (int i = 0; i < VEC; ++i)
                if (c0 + i < k) row[c0 + i] = at(i);
        }
    }
    __device__ __forceinline__ void store_from(float *row, int c0, int k) const
    {
        if (c0 >= k) {
            store(row + c0);
        } else {
#pragma unroll
            for (int i = 0; i < VEC; ++i)
                if (c0 + i >= k) row[c0 + i] = at(i);
        }
    }
    __device__ __forceinline__ void store_elements(float *p) const // where p is aligned as a float only
    {
#pragma unroll
        for (int i = 0; i < VEC; ++i) p[i] = at(i);
    }
};

// Thread layout: a block owns `rows_per_block` consecutive rows of ONE mesh; thread t owns column group
// (t % groups) for rows (t / groups), (t / groups) + rows_in_flight, ...  so that
//   * a wave reads/writes contiguous runs of a row (coalesced),
//   * a thread's column group is FIXED, which lets the backward kernel accumulate the bias
//     gradient (column sums of g) in registers and emit one partial per block -- reduced by a
//     second tiny kernel in a fixed order (deterministic, no atomics).
// Neighbour gathers are issued in batches of NB: first all (col, val) pairs of the batch, then
// all neighbour rows, so a row costs two memory round trips instead of two per neighbour.
constexpr int GCN_NB = 8;         // neighbours fetched per batch
constexpr int GCN_BWD_ITERS = 2;  // rows per thread in the backward (halves the bias-gradient partials)

// Where a term's operand and its activation derivative are read from.
struct Source {
    const float *x;             // support (forward) or grad_out (backward); null in the head's backward
    const float *saved;         // backward: forward output (act' where there is no sign mask)
    const unsigned short *mask; // MASK: one word per (row, aggregated float4 j of kg); bit e <-> element e of that float4
    int kg, j;
    const float *head;          // HEAD backward: grad_pos [rows, 3]; the upstream gradient is [head_scale * grad_pos | 0 ...]
    float head_scale;
    int c;
};

// THE NEIGHBOUR TERM, and every other element a thread reads with the derivative folded in: VEC columns of one row, in two
// halves.  Callers issue term_load for a whole round of rows before the first term_finish / term_add: a round is then one
// memory round trip.  The three values of a term (operand, saved output, sign bits) live in the caller's arrays, one array
// per value as the kernels always had them: what a variant does not read is never loaded and costs no register.
template <int VEC_, int ACT_, bool BACKWARD_, bool MASK_ = false, bool HEAD_ = false>
struct TermKind {
    static_assert((!MASK_ && !HEAD_) || VEC_ == 4, "sign mask and head are the fast kernel's");
    static constexpr int VEC = VEC_, ACT = ACT_;
    static constexpr bool BACKWARD = BACKWARD_, MASK = MASK_, HEAD = HEAD_;
};

// load half: the operand into v (HEAD backward: synthesised from grad_pos, non-zero in the row's first float4 only) and, in the
// backward, where act' comes from: the sign-mask word into bits, or the saved output into out
template <class KIND, int VEC>
__device__ __forceinline__ void term_load(Pack<VEC> &v, Pack<VEC> &out, unsigned &bits, const Source &s, int64_t row, int col)
{
    if (KIND::BACKWARD && KIND::HEAD) {
        v = Pack<VEC>::zero();
        if (col == 0) {
            const float *gp = s.head + row * 3;
#pragma unroll
            for (int i = 0; i < 3 && i < VEC; ++i) v.at(i) = s.head_scale * gp[i];
        }
    } else {
        v.load(s.x + row * s.c + col);
    }
    if (KIND::BACKWARD && KIND::MASK) bits = s.mask[row * s.kg + s.j];
    else if (KIND::BACKWARD && KIND::ACT != ACT_NONE) out.load(s.saved + row * s.c + col);
}

// finish half: the derivative applied to the operand (in place) ...
template <class KIND, int VEC>
__device__ __forceinline__ void term_finish(Pack<VEC> &v, const Pack<VEC> &out, unsigned bits)
{
    if (KIND::BACKWARD && KIND::MASK) v.keep_where(bits);
    else if (KIND::BACKWARD && KIND::ACT != ACT_NONE) v.template act_bwd_from<KIND::ACT>(out);
}

// ... and acc += w * v: the one statement of the sum (callers skip padded slots, they do not multiply by zero)
template <class KIND, int VEC>
__device__ __forceinline__ void term_add(Pack<VEC> &acc, float w, Pack<VEC> &v, const Pack<VEC> &out, unsigned bits)
{
    term_finish<KIND>(v, out, bits);
    acc.add_scaled(w, v);
}

// The thread's own element of `row` (pass-through value and / or bias-gradient term).
template <class KIND, int VEC>
__device__ __forceinline__ void own_element(Pack<VEC> &own, const Source &s, int64_t row, int col)
{
    Pack<VEC> out;
    unsigned bits = 0u;
    term_load<KIND>(own, out, bits, s, row, col);
    term_finish<KIND>(own, out, bits);
}

// A CSR run [e, e1) of (col, val) added to acc in order, GCN_NB entries per batch: the pairs first, then the rows, then
// the sum; the slots past the end read the thread's own row and contribute nothing.
template <class KIND, int VEC>
__device__ __forceinline__ void add_csr_run(Pack<VEC> &acc, const Source &s, const int *col, const float *val, int e, int e1,
                                            int64_t mesh_row0, int64_t row, int c0)
{
    for (; e < e1; e += GCN_NB) {
        int64_t nb[GCN_NB];
        float w[GCN_NB];
#pragma unroll
        for (int j = 0; j < GCN_NB; ++j) {
            const bool in = e + j < e1;
            nb[j] = in ? mesh_row0 + col[e + j] : row;
            w[j] = in ? val[e + j] : 0.f;
        }
        Pack<VEC> sv[GCN_NB], ov[GCN_NB];
        unsigned bits[GCN_NB] = {};
#pragma unroll
        for (int j = 0; j < GCN_NB; ++j) term_load<KIND>(sv[j], ov[j], bits[j], s, nb[j], c0);
#pragma unroll
        for (int j = 0; j < GCN_NB; ++j)
            if (e + j < e1) term_add<KIND>(acc, w[j], sv[j], ov[j], bits[j]); // keep the CSR order of the sum
    }
}

// Row r of a [nv][W] neighbour table (col -1 = padding), 16 bytes at a time.
template <int W>
__device__ __forceinline__ void load_table_row(const int *col, const float *val, int r, int (&nb)[W], float (&w)[W])
{
#pragma unroll
    for (int n = 0; n < W; n += 4) {
        const int4 ci = *reinterpret_cast<const int4 *>(col + (size_t)r * W + n);
        const float4 wi = *reinterpret_cast<const float4 *>(val + (size_t)r * W + n);
        nb[n] = ci.x, nb[n + 1] = ci.y, nb[n + 2] = ci.z, nb[n + 3] = ci.w;
        w[n] = wi.x, w[n + 1] = wi.y, w[n + 2] = wi.z, w[n + 3] = wi.w;
    }
}

// The W table slots of row r: all their loads (a padded slot reads row r itself), then the sum in slot order == CSR order.
template <class KIND, int W, int VEC>
__device__ __forceinline__ void load_table_slots(Pack<VEC> (&sv)[W], Pack<VEC> (&ov)[W], unsigned (&bits)[W], const Source &s,
                                                 const int (&nb)[W], int64_t mesh_row0, int r, int c0)
{
#pragma unroll
    for (int n = 0; n < W; ++n) term_load<KIND>(sv[n], ov[n], bits[n], s, mesh_row0 + (nb[n] >= 0 ? nb[n] : r), c0);
}

template <class KIND, int W, int VEC>
__device__ __forceinline__ void add_table_slots(Pack<VEC> &acc, Pack<VEC> (&sv)[W], const Pack<VEC> (&ov)[W], const unsigned (&bits)[W],
                                                const int (&nb)[W], const float (&w)[W])
{
#pragma unroll
    for (int n = 0; n < W; ++n)
        if (nb[n] >= 0) term_add<KIND>(acc, w[n], sv[n], ov[n], bits[n]);
}

// Block partial of the bias gradient in the row-major layouts: the threads' column sums through lds [rows_in_flight][c], row 0's
// threads add them in row order (fixed summation order) into partial_row [c].
template <int VEC>
__device__ __forceinline__ void write_colsum_partial(float *lds, const Pack<VEC> &colsum, bool active, int rl, int rows_in_flight,
                                                     int c, int c0, float *partial_row)
{
    if (active) colsum.store_elements(lds + rl * c + c0);
    __syncthreads();
    if (active && rl == 0) {
#pragma unroll
        for (int i = 0; i < VEC; ++i) {
            float t = 0.f;
            for (int l = 0; l < rows_in_flight; ++l) t += lds[l * c + c0 + i];
            partial_row[c0 + i] = t;
        }
    }
}

template <int VEC, int ACT, bool BACKWARD>
__global__ __launch_bounds__(GCN_THREADS) void zn_aggregate_kernel(GcnArgs a, int groups, int rows_in_flight,
                                                                    int rows_per_block, float *colsum_partial)
{
    using KIND = TermKind<VEC, ACT, BACKWARD>;
    extern __shared__ float lds_colsum[]; // [rows_in_flight][c], backward with colsum only
    const int g = threadIdx.x % groups;
    const int rl = threadIdx.x / groups;
    const int c0 = g * VEC;
    const bool active = rl < rows_in_flight;
    // grid = (row chunks of one mesh, meshes): no integer division on the row index
    const int r_begin = blockIdx.x * rows_per_block;
    const int r_end = min(r_begin + rows_per_block, a.nv);
    const int64_t mesh_row0 = (int64_t)blockIdx.y * a.nv; // first row of this mesh
    const Source src{.x = a.x, .saved = a.saved, .c = a.c};

    Pack<VEC> colsum = Pack<VEC>::zero();

    if (active) {
        for (int r = r_begin + rl; r < r_end; r += rows_in_flight) {
            const int64_t row = mesh_row0 + r;
            Pack<VEC> acc, own;
            const bool pass = c0 + VEC > a.k; // the group holds pass-through columns (all of them, or -- when k is not
                                              // a multiple of VEC -- the tail of the group that straddles column k)
            if (BACKWARD || pass) own_element<KIND>(own, src, row, c0); // pass-through value and/or bias-gradient term
            if (c0 < a.k) {
                acc = Pack<VEC>::zero();
                add_csr_run<KIND>(acc, src, a.col, a.val, a.rowptr[r], a.rowptr[r + 1], mesh_row0, row, c0);
                if (pass) acc.take_from(own, a.k - c0); // straddling group: the gathered values of columns >= k are discarded
            } else {
                acc = own;
            }
            if (BACKWARD) colsum.add(own);
            else acc.template bias_act<ACT>(a.bias, c0);
            acc.store(a.y + row * a.c + c0);
        }
    }

    if (BACKWARD && colsum_partial) // block partial of the bias gradient, fixed summation order
        write_colsum_partial(lds_colsum, colsum, active, rl, rows_in_flight, a.c, c0,
                             colsum_partial + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * a.c);
}

// grad_bias[c] = sum over blocks of partial[blk][c].  16 columns x 64 block-lanes per workgroup:
// lane l adds blocks l, l+64, ... (independent loads, pipelined), then the 64 lane sums are added
// in ascending lane order -- a fixed tree, so the result is bit-reproducible.
constexpr int CS_COLS = 16, CS_LANES = 64;
__device__ __forceinline__ void reduce_partials(float (&part)[CS_LANES][CS_COLS], int blocks, int c, const float *partial, float *out)
{
    const int cl = threadIdx.x % CS_COLS, lane = threadIdx.x / CS_COLS;
    const int col = blockIdx.x * CS_COLS + cl;
    float t = 0.f;
    if (col < c) {
#pragma unroll 8
        for (int b = lane; b < blocks; b += CS_LANES) t += partial[(size_t)b * c + col];
    }
    part[lane][cl] = t;
    __syncthreads();
    if (lane == 0 && col < c) {
        float acc = 0.f;
        for (int l = 0; l < CS_LANES; ++l) acc += part[l][cl];
        out[col] = acc;
    }
}

__global__ __launch_bounds__(CS_COLS *CS_LANES) void colsum_final_kernel(int blocks, int c, const float *partial,
                                                                         float *out)
{
    __shared__ float part[CS_LANES][CS_COLS];
    reduce_partials(part, blocks, c, partial, out);
}

// The same reduction for several pending bias gradients in ONE launch (blockIdx.y = job): a backward pass through N
// layers leaves N sets of partials, and N separate 4.7 us launches are 5 % of the reference's training-shape step.
struct ColsumJobs {
    const float *partial[GEOM_COLSUM_MAX_JOBS];
    float *out[GEOM_COLSUM_MAX_JOBS];
    int blocks[GEOM_COLSUM_MAX_JOBS], c[GEOM_COLSUM_MAX_JOBS];
};

__global__ __launch_bounds__(CS_COLS *CS_LANES) void colsum_batch_kernel(ColsumJobs jobs)
{
    __shared__ float part[CS_LANES][CS_COLS];
    const int job = blockIdx.y;
    if ((int)blockIdx.x * CS_COLS >= jobs.c[job]) return; // a job narrower than the widest one
    reduce_partials(part, jobs.blocks[job], jobs.c[job], jobs.partial[job], jobs.out[job]);
}

struct GcnGeometry {
    int groups, rows_in_flight, rows_per_block;
    int chunks;     // blocks per mesh (grid.x)
    int64_t blocks; // chunks * meshes
};

inline GcnGeometry gcn_geometry(int b, int nv, int c, int vec, bool backward)
{
    GcnGeometry g;
    g.groups = c / vec;
    g.rows_in_flight = g.groups >= GCN_THREADS ? 1 : GCN_THREADS / g.groups;
    g.rows_per_block = g.rows_in_flight * (backward ? GCN_BWD_ITERS : 1);
    g.chunks = (nv + g.rows_per_block - 1) / g.rows_per_block;
    g.blocks = (int64_t)g.chunks * b;
    return g;
}

inline bool gcn_vec4(int c, int /*k*/) { return c % 4 == 0; } // any k: the group straddling column k is mixed

// ---- what the dispatchers below share -----------------------------------------------------------------------------------------
inline int check_sizes(int b, int nv, int c, int k) { return (b < 0 || nv < 0 || c < 0 || k < 0 || k > c) ? GEOM_EINVAL : 0; }

// What a backward needs beyond its operands: the forward output wherever an activation's derivative is read from it
// (has_saved: `saved`, or the sign mask on the route that has one), and scratch for the bias gradient's partials.
template <bool BACKWARD>
int check_gradient_operands(int act, bool has_saved, const float *grad_bias, const float *scratch)
{
    return ((BACKWARD && act != ACT_NONE && !has_saved) || (grad_bias && !scratch)) ? GEOM_EINVAL : 0;
}

// After an aggregation launch: a backward that left `blocks` rows of column-sum partials reduces them into grad_bias in fixed
// order.  grad_bias == null: the partials stay un-reduced (geom_colsum_batch_f32 finishes them at the end of the pass).
inline int finish_launch(bool backward, int64_t blocks, int c, const float *partial, float *grad_bias, hipStream_t s)
{
    if (backward && partial && grad_bias)
        hipLaunchKernelGGL(colsum_final_kernel, dim3((c + CS_COLS - 1) / CS_COLS), dim3(CS_COLS * CS_LANES), 0, s, (int)blocks, c,
                           partial, grad_bias);
    return geom::launch_status();
}

// Run-time values as template arguments: f is called with the value as a std::integral_constant.  Activation code (false: no
// such code, f not called), table width 8 / 16 (the dispatcher admits no other), vector width 4 / 2 / 1.
template <int V>
using Const = std::integral_constant<int, V>;

template <class F>
bool with_act(int act, F &&f)
{
    switch (act) {
    case ACT_NONE: f(Const<ACT_NONE>{}); return true;
    case ACT_RELU: f(Const<ACT_RELU>{}); return true;
    case ACT_ELU: f(Const<ACT_ELU>{}); return true;
    default: return false;
    }
}

template <class F>
void with_width(int w, F &&f) { w == 8 ? f(Const<8>{}) : f(Const<16>{}); }

template <class F>
void with_vec(int vec, F &&f) { vec == 4 ? f(Const<4>{}) : vec == 2 ? f(Const<2>{}) : f(Const<1>{}); }

template <int VEC, bool BACKWARD>
int launch(const GcnArgs &a, int act, float *colsum_partial, float *grad_bias, void *stream)
{
    const int meshes = (int)(a.rows / a.nv);
    const GcnGeometry geo = gcn_geometry(meshes, a.nv, a.c, VEC, BACKWARD);
    if (geo.groups > GCN_THREADS) return GEOM_ETOOBIG; // > 1024 channels (VEC=4): not a 0N-GCN shape
    if (meshes > 65535 || geo.blocks > 0x7fffffffLL) return GEOM_ETOOBIG;
    dim3 grid((unsigned)geo.chunks, (unsigned)meshes), block(GCN_THREADS);
    const size_t lds = (BACKWARD && colsum_partial) ? (size_t)geo.rows_in_flight * a.c * sizeof(float) : 0;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const bool known = with_act(act, [&](auto ACT) {
        hipLaunchKernelGGL((zn_aggregate_kernel<VEC, decltype(ACT)::value, BACKWARD>), grid, block, lds, s, a, geo.groups,
                           geo.rows_in_flight, geo.rows_per_block, colsum_partial);
    });
    return known ? finish_launch(BACKWARD, geo.blocks, a.c, colsum_partial, grad_bias, s) : GEOM_EINVAL;
}

// ---------------------------------------------------------------------------------------
// ELL fast path (k % 4 == 0, C == k * (NC + 1) with NC = 2 (split 3) or 9 (split 10); the first W = 8 / 16
// entries of every row in a fixed-stride table, the few longer rows -- the two 33-entry poles of the reference's
// training template 482.obj -- continue in a short CSR tail: every hidden layer of the reference models on a
// triangle mesh).
//
// Thread (row, j) owns the aggregated float4 j of the row AND the NC pass-through float4s
// j + (k/4)*i of the same row.  Compared with the generic kernel above:
//   * every lane gathers (no wave where 2/3 of the lanes wait for the gathering third),
//     b*V*k/4 threads fit the chip in ONE resident round;
//   * neighbour indices/weights sit at a fixed stride (ELL, -1 padded): no rowptr round trip, the
//     index loads and the thread's own pass-through loads are issued together, then all W
//     neighbour rows -- two memory round trips per thread;
//   * the thread stores NC + 1 float4s; in the backward it also owns the bias-gradient terms of
//     those columns, reduced per workgroup through LDS (fixed order) into one partial per block.
struct EllArgs {
    const int *col;     // [nv][W], -1 = padding
    const float *val;   // [nv][W]
    const float *x, *bias, *saved;
    float *y;
    int nv, c, k;
    unsigned short *mask; // ReLU sign bits, one word per thread: bit 4*i + e <-> element e of the thread's float4 i
    // rows longer than W (the 33-entry poles of the reference's 482.obj): entries W.. of every row in CSR form,
    // summed after the table slots, i.e. still in CSR order.  over_ptr == null: no row is longer than W.
    const int *over_ptr, *over_col;
    const float *over_val;
    int b, chunks; // meshes, workgroups per mesh (filled in by the dispatcher)
    // HEAD (the layer whose three leading output channels are a coordinate update, GEOMetrics.py:121,126,131):
    //   forward : head_out[row] = head_in[row] + head_scale * out[row, :3]   (base positions in, new positions out)
    //   backward: grad_out is not read at all -- it is [head_scale * head_in[row, :3] | 0 ...] by construction
    //             (head_in = grad_pos [rows, 3]); x may be null
    const float *head_in;
    float *head_out;
    float head_scale;
};

// MASK (ReLU, NC == 2 only): the forward also stores the sign of every output element as one bit (12 bits per
// thread -> 0.66 MB per layer at the BASELINE shard), and the backward takes relu' from those bits instead of
// re-reading the 15.7 MB forward output: 47 -> 32 MB of traffic for the backward launch.
template <int ACT, bool BACKWARD, int W, int NC, bool MASK = false, bool HEAD = false>
__global__ __launch_bounds__(GCN_THREADS) void zn_aggregate_ell_kernel(EllArgs a, int rows_per_block, int iters,
                                                                        float *colsum_partial)
{
    static_assert(!MASK || (ACT == ACT_RELU && NC == 2), "the sign mask is the ReLU / split-3 fast path");
    extern __shared__ float lds_cs[]; // [rows_per_block][c]
    const int kg = a.k >> 2;                         // aggregated float4 groups per row
    const int j = threadIdx.x % kg;
    const int rl = threadIdx.x / kg;
    // a mesh's workgroups share one XCD (geom::xcd_assign): the neighbour rows every thread gathers -- each row of the
    // k-slice is read by ~7 workgroups -- then hit that XCD's L2 instead of being fetched into all eight
    int mesh_i, chunk_i;
    if (!geom::xcd_assign(blockIdx.x, a.b, a.chunks, mesh_i, chunk_i)) return;
    const int64_t mesh_row0 = (int64_t)mesh_i * a.nv;
    const int c0 = 4 * j;
    using KIND = TermKind<4, ACT, BACKWARD, MASK, HEAD>;
    const Source src{.x = a.x, .saved = a.saved, .mask = a.mask, .kg = kg, .j = j, .head = a.head_in, .head_scale = a.head_scale, .c = a.c};
    // `iters` consecutive row tiles per workgroup (the backward uses 2: half the bias-gradient partials to reduce)
    float4 csum[NC + 1]; // bias-gradient terms of this thread's columns over its rows (backward)
#pragma unroll
    for (int i = 0; i <= NC; ++i) csum[i] = make_float4(0.f, 0.f, 0.f, 0.f);

    for (int it = 0; it < iters; ++it) {
    const int r = (chunk_i * iters + it) * rows_per_block + rl;
    const bool active = rl < rows_per_block && r < a.nv;
    float4 own[NC + 1]; // [0] = own aggregated-slot element (backward only), [1..NC] = pass-through
#pragma unroll
    for (int i = 0; i <= NC; ++i) own[i] = make_float4(0.f, 0.f, 0.f, 0.f);

    if (active) {
        const int64_t row = mesh_row0 + r;
        const float *xrow = a.x + row * a.c;
        // round trip 1: indices, weights and the thread's own elements
        int nb[W];
        float w[W];
        load_table_row<W>(a.col, a.val, r, nb, w);
        constexpr int TAIL = (ACT == ACT_NONE && NC == 2) ? 16 : 8; // entries of a long row per round (below)
        int e0 = 0, e1 = 0; // the row's entries beyond the table width, in the CSR tail
        if (a.over_ptr) e0 = a.over_ptr[r], e1 = a.over_ptr[r + 1];
        unsigned own_bits = 0u;
        if (BACKWARD && MASK) own_bits = a.mask[row * kg + j];
#pragma unroll
        for (int i = BACKWARD ? 0 : 1; i <= NC; ++i) {
            if (BACKWARD && HEAD) { // the upstream gradient is [scale * grad_pos | 0]: only the row's first float4 is non-zero
                if (i == 0 && j == 0) {
                    const float *gp = a.head_in + row * 3;
                    own[0] = make_float4(a.head_scale * gp[0], a.head_scale * gp[1], a.head_scale * gp[2], 0.f);
                }
            } else
            own[i] = *reinterpret_cast<const float4 *>(xrow + c0 + a.k * i);
            if (BACKWARD && MASK) {
                const unsigned m = own_bits >> (4 * i);
                own[i].x = (m & 1u) ? own[i].x : 0.f;
                own[i].y = (m & 2u) ? own[i].y : 0.f;
                own[i].z = (m & 4u) ? own[i].z : 0.f;
                own[i].w = (m & 8u) ? own[i].w : 0.f;
            } else if (BACKWARD && ACT != ACT_NONE) {
                const float4 o = *reinterpret_cast<const float4 *>(a.saved + row * a.c + c0 + a.k * i);
                own[i].x = act_bwd<ACT>(own[i].x, o.x);
                own[i].y = act_bwd<ACT>(own[i].y, o.y);
                own[i].z = act_bwd<ACT>(own[i].z, o.z);
                own[i].w = act_bwd<ACT>(own[i].w, o.w);
            }
        }
        // round trip 2: the neighbour rows of the aggregated slot
        Pack<4> sv[W], ov[W];
        unsigned nbits[W] = {};
        load_table_slots<KIND>(sv, ov, nbits, src, nb, mesh_row0, r, c0);
        int tcol[TAIL];
        float tval[TAIL];
        if (e0 < e1) { // a long row: the indices of its first TAIL extra entries travel with the neighbour rows
#pragma unroll
            for (int t = 0; t < TAIL; ++t) {
                const int ee = e0 + t < e1 ? e0 + t : e1 - 1;
                tcol[t] = a.over_col[ee];
                tval[t] = a.over_val[ee];
            }
        }
        Pack<4> acc = Pack<4>::zero();
        add_table_slots<KIND>(acc, sv, ov, nbits, nb, w); // ELL order == CSR order of the row
        // the row's entries beyond the table width (wave-divergent only at the few long rows).  TAIL entries per round:
        // their rows in one round trip, the NEXT round's indices requested meanwhile (one entry at a time the 25 extra
        // entries of a 482.obj pole cost 50 dependent round trips, and the two pole rows set the launch time)
        for (int e = e0; e < e1; e += TAIL) {
            int64_t nrow[TAIL];
            float wv[TAIL];
            Pack<4> tv[TAIL], to[TAIL];
            unsigned tb[TAIL] = {};
#pragma unroll
            for (int t = 0; t < TAIL; ++t) {
                nrow[t] = mesh_row0 + tcol[t];
                wv[t] = tval[t];
                term_load<KIND>(tv[t], to[t], tb[t], src, nrow[t], c0);
            }
            if (e + TAIL < e1) {
#pragma unroll
                for (int t = 0; t < TAIL; ++t) {
                    const int ee = e + TAIL + t < e1 ? e + TAIL + t : e1 - 1;
                    tcol[t] = a.over_col[ee];
                    tval[t] = a.over_val[ee];
                }
            }
#pragma unroll
            for (int t = 0; t < TAIL; ++t)
                if (e + t < e1) term_add<KIND>(acc, wv[t], tv[t], to[t], tb[t]); // still in CSR order
        }
        float *yrow = a.y + row * a.c;
        unsigned sign_bits = 0u;
#pragma unroll
        for (int i = 0; i <= NC; ++i) {
            Pack<4> v;
            v.v = i == 0 ? acc.v : own[i];
            if (!BACKWARD) {
                v.template bias_act<ACT, true>(a.bias, c0 + a.k * i);
                if (MASK) sign_bits |= v.positive_bits() << (4 * i);
            }
            v.store(yrow + c0 + a.k * i);
            if (!BACKWARD && HEAD && i == 0 && j == 0) { // new positions = base + scale * the three leading channels
                const float *bp = a.head_in + row * 3;
                float *pp = a.head_out + row * 3;
#pragma unroll
                for (int e = 0; e < 3; ++e) pp[e] = bp[e] + a.head_scale * v.at(e);
            }
        }
        if (!BACKWARD && MASK) a.mask[row * kg + j] = (unsigned short)sign_bits;
    }
    if (BACKWARD) {
#pragma unroll
        for (int i = 0; i <= NC; ++i)
            csum[i].x += own[i].x, csum[i].y += own[i].y, csum[i].z += own[i].z, csum[i].w += own[i].w;
    }
    } // row tiles

    if (BACKWARD && colsum_partial) {
        if (rl < rows_per_block) {
#pragma unroll
            for (int i = 0; i <= NC; ++i)
                *reinterpret_cast<float4 *>(lds_cs + rl * a.c + c0 + a.k * i) = csum[i]; // zeros for inactive rows
        }
        __syncthreads();
        for (int c = threadIdx.x; c < a.c; c += GCN_THREADS) {
            float t = 0.f;
            for (int l = 0; l < rows_per_block; ++l) t += lds_cs[l * a.c + c];
            colsum_partial[((size_t)mesh_i * a.chunks + chunk_i) * a.c + c] = t;
        }
    }
}

// Which table kernel takes a shape (asked by the dispatcher and the two size functions): none = the CSR kernel at the top; the
// kernel above at split 3 (the one with the sign mask and the head) / split 10; zn_aggregate_ell_any_kernel below, any width.
enum EllRoute { ELL_NONE, ELL_FAST3, ELL_FAST10, ELL_ANY };

inline int ell_any_vec(int c) { return c % 4 == 0 ? 4 : c % 2 == 0 ? 2 : 1; }
inline int ell_nc(int c, int k) { return (k > 0 && k % 4 == 0 && c % k == 0) ? c / k - 1 : -1; } // pass-through float4s per aggregated one

inline EllRoute ell_route(int c, int k, int w)
{
    if (w != 8 && w != 16) return ELL_NONE;
    const int nc = ell_nc(c, k);
    if ((nc == 2 || nc == 9) && (k >> 2) <= GCN_THREADS) return nc == 2 ? ELL_FAST3 : ELL_FAST10;
    return (c > 0 && c / ell_any_vec(c) <= GCN_THREADS) ? ELL_ANY : ELL_NONE;
}

// rows of one tile (a thread per aggregated float4 of a row), row tiles per workgroup, workgroups per mesh, chunks * meshes
struct EllGeometry { int rows_per_block, iters, chunks; int64_t blocks; };

inline EllGeometry ell_geometry(int b, int nv, int k, bool backward)
{
    EllGeometry g;
    g.rows_per_block = GCN_THREADS / (k >> 2);
    // row tiles per workgroup (measured at the BASELINE shard, us: forward 8.1 / 8.4 / 9.2 / 11.1 for 1-4 tiles --
    // one row per thread keeps the most loads in flight; backward incl. the bias reduction 14.6 / 12.8 / 13.7 / 14.8)
    g.iters = backward ? 2 : 1;
    g.chunks = (nv + g.rows_per_block * g.iters - 1) / (g.rows_per_block * g.iters);
    g.blocks = (int64_t)g.chunks * b;
    return g;
}

// ---------------------------------------------------------------------------------------
// ELL table, ANY width and split: the unbatched ZERON_GCN layers of the mesh encoder (reference layers.py:34-41 with
// models.py:299-348's widths: c = 60 ... 300, k = c / 10 = 6 ... 30 -- neither k % 4 == 0 nor c % k == 0 holds for most).
// The thread layout of the generic CSR kernel at the top of this file (one thread = VEC consecutive columns of a row, the
// group that straddles column k is mixed) with the neighbour entries from the fixed-stride table instead of the
// rowptr -> (col, val) chain: two dependent round trips per gathering thread instead of three, the table read issued with
// the thread's own elements.  VEC = 4 / 2 / 1 by the divisibility of c (150, 210, 250 are even, not multiples of 4).
// Workgroups run several row tiles (forward: keeps the grid at a few thousand workgroups; backward: at most ~1024
// bias-gradient partials to reduce -- 3072 partial rows of 300 columns cost an 8 us reduction launch per layer).
// Summation order = table order = CSR order: bit-identical to the generic kernel.
// ---------------------------------------------------------------------------------------
template <int VEC, int ACT, bool BACKWARD, int W>
__global__ __launch_bounds__(GCN_THREADS) void zn_aggregate_ell_any_kernel(EllArgs a, int groups, int rows_in_flight, int rows_per_block,
                                                                            float *colsum_partial)
{
    using KIND = TermKind<VEC, ACT, BACKWARD>;
    extern __shared__ float lds_colsum[]; // [rows_in_flight][c], backward with colsum only
    const int r_begin = blockIdx.x * rows_per_block;
    const int r_end = min(r_begin + rows_per_block, a.nv);
    const int64_t mesh_row0 = (int64_t)blockIdx.y * a.nv;
    const Source src{.x = a.x, .saved = a.saved, .c = a.c};

    // ---- the aggregated columns: COMPACT gather threads.  Item (row, j): group j < kgs of the row (kgs = the groups that hold
    // an aggregated column, the straddling one included); every lane of a wave gathers -- with the gathers left to the few
    // lanes of a row-major layout that own aggregated columns (8 of 75 at c = 300) a wave issued its 12 memory instructions
    // for 128 useful bytes each, and the launch took 18.7 us against 10.9 for the copy alone (tools/probe/agg_any_probe.py)
    const int kgs = (a.k + VEC - 1) / VEC;
    for (int item = threadIdx.x; item < (r_end - r_begin) * kgs; item += GCN_THREADS) {
        const int r = r_begin + item / kgs, c0 = (item % kgs) * VEC;
        const int64_t row = mesh_row0 + r;
        int nb[W];
        float w[W];
        load_table_row<W>(a.col, a.val, r, nb, w); // round trip 1: the row's table entries
        int e0 = 0, e1 = 0;
        if (a.over_ptr) e0 = a.over_ptr[r], e1 = a.over_ptr[r + 1];
        Pack<VEC> sv[W], ov[W];
        unsigned nbits[W] = {};
        load_table_slots<KIND>(sv, ov, nbits, src, nb, mesh_row0, r, c0); // round trip 2: the neighbour rows
        Pack<VEC> acc = Pack<VEC>::zero();
        add_table_slots<KIND>(acc, sv, ov, nbits, nb, w);
        add_csr_run<KIND>(acc, src, a.over_col, a.over_val, e0, e1, mesh_row0, row, c0); // a row longer than the table
        // (the straddling group takes bias[c0 + i] for its columns >= k as well: in bounds, VEC divides c, and store_below drops them)
        if (!BACKWARD) acc.template bias_act<ACT>(a.bias, c0);
        acc.store_below(a.y + row * a.c, c0, a.k); // (the straddling group's other elements: the pass-through threads')
    }

    // ---- everything else, row-major: thread (rl, g) owns VEC consecutive columns of rows rl, rl + rows_in_flight, ...: the
    // pass-through columns (copy + bias + activation / derivative) and, in the backward, the bias-gradient terms of ALL columns
    const int g = threadIdx.x % groups;
    const int rl = threadIdx.x / groups;
    const int c0 = g * VEC;
    const bool active = rl < rows_in_flight;
    const bool pass = c0 + VEC > a.k; // pass-through columns in the group (all, or the tail of the straddling group)

    Pack<VEC> colsum = Pack<VEC>::zero();

    if (active && (BACKWARD || pass)) {
        for (int r = r_begin + rl; r < r_end; r += rows_in_flight) {
            const int64_t row = mesh_row0 + r;
            Pack<VEC> own;
            own_element<KIND>(own, src, row, c0);
            if (BACKWARD) colsum.add(own);
            else own.template bias_act<ACT>(a.bias, c0);
            own.store_from(a.y + row * a.c, c0, a.k);
        }
    }

    if (BACKWARD && colsum_partial) // block partial of the bias gradient, fixed summation order
        write_colsum_partial(lds_colsum, colsum, active, rl, rows_in_flight, a.c, c0,
                             colsum_partial + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * a.c);
}

inline GcnGeometry ell_any_geometry(int b, int nv, int c, bool backward)
{
    GcnGeometry g;
    g.groups = c / ell_any_vec(c);
    g.rows_in_flight = GCN_THREADS / g.groups;
    // row tiles per workgroup: at most ~1024 workgroups in either direction (backward: = bias-gradient partials to reduce;
    // forward: a 300-column copy alone ran at 3.3 TB/s as 3072 two-tile workgroups and at 4.0 as 1024 six-tile ones)
    const int64_t tiles = ((int64_t)b * nv + g.rows_in_flight - 1) / g.rows_in_flight;
    int64_t iters = (tiles + 1023) / 1024;
    const int64_t lo = backward ? GCN_BWD_ITERS : 1, hi = 64;
    iters = iters < lo ? lo : iters > hi ? hi : iters;
    g.rows_per_block = g.rows_in_flight * (int)iters;
    g.chunks = (nv + g.rows_per_block - 1) / g.rows_per_block;
    g.blocks = (int64_t)g.chunks * b;
    return g;
}

// The table kernels' dispatcher.  Its checks are the CSR dispatcher's with the table's own in between; where the two differ:
// c == 0 has no route here (only the CSR dispatcher calls that shape empty), relu' comes from the sign mask where there is one,
// the fast kernel reads its bias as float4s too, and the mesh axis is checked before the geometry (it does not depend on it).
template <bool BACKWARD>
int dispatch_ell(EllArgs a, int b, int w, int act, float *grad_bias, float *scratch, void *stream)
{
    if (const int code = check_sizes(b, a.nv, a.c, a.k)) return code;
    const EllRoute route = ell_route(a.c, a.k, w);
    const bool fast = route == ELL_FAST3 || route == ELL_FAST10;
    if (route == ELL_NONE || (!fast && (a.head_in || a.mask))) return GEOM_EUNSUPPORTED; // head and sign mask: the fast kernel's
    if (b == 0 || a.nv == 0) return 0;
    if (!a.col || !a.val || !a.y || (!a.x && !(BACKWARD && a.head_in))) return GEOM_EINVAL;
    // head mode: split 3, ReLU with the sign mask or no activation; the forward also needs head_out
    if (a.head_in && (route != ELL_FAST3 || !((act == ACT_RELU && a.mask) || act == ACT_NONE) || (!BACKWARD && !a.head_out)))
        return GEOM_EUNSUPPORTED;
    if (a.mask && !(act == ACT_RELU && route == ELL_FAST3)) return GEOM_EINVAL; // sign mask: ReLU, split 3 only
    if (const int code = check_gradient_operands<BACKWARD>(act, a.saved || a.mask, grad_bias, scratch)) return code;
    if (a.over_ptr && (!a.over_col || !a.over_val)) return GEOM_EINVAL;
    // the table rows are read 16 bytes at a time; the operands as float4s, or (any width) VEC floats at a time: VEC divides c
    if ((((uintptr_t)a.col | (uintptr_t)a.val) % 16) != 0) return GEOM_EINVAL;
    if ((((uintptr_t)a.x | (uintptr_t)a.y | (uintptr_t)a.saved | (uintptr_t)(fast ? a.bias : nullptr)) % (fast ? 16 : 4 * ell_any_vec(a.c))) != 0)
        return GEOM_EINVAL;
    if (b > 65535) return GEOM_ETOOBIG;
    float *partial = scratch; // with grad_bias == null the partials stay un-reduced (geom_colsum_batch_f32 finishes them)
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (!fast) {
        const GcnGeometry geo = ell_any_geometry(b, a.nv, a.c, BACKWARD);
        const size_t lds = (BACKWARD && partial) ? (size_t)geo.rows_in_flight * a.c * sizeof(float) : 0;
        const dim3 grid((unsigned)geo.chunks, (unsigned)b);
        const bool known = with_act(act, [&](auto ACT) { with_width(w, [&](auto W) { with_vec(ell_any_vec(a.c), [&](auto VEC) {
            hipLaunchKernelGGL((zn_aggregate_ell_any_kernel<decltype(VEC)::value, decltype(ACT)::value, BACKWARD, decltype(W)::value>),
                               grid, dim3(GCN_THREADS), lds, s, a, geo.groups, geo.rows_in_flight, geo.rows_per_block, partial);
        }); }); });
        return known ? finish_launch(BACKWARD, geo.blocks, a.c, partial, grad_bias, s) : GEOM_EINVAL;
    }
    const EllGeometry geo = ell_geometry(b, a.nv, a.k, BACKWARD);
    const size_t lds = (BACKWARD && partial) ? (size_t)geo.rows_per_block * a.c * sizeof(float) : 0;
    a.b = b, a.chunks = geo.chunks;
    const dim3 grid(geom::xcd_grid(b, geo.chunks));
    const bool known = with_act(act, [&](auto ACT) { with_width(w, [&](auto W) {
        constexpr int A = decltype(ACT)::value;
        auto go = [&](auto NC, auto MASK, auto HEAD) {
            hipLaunchKernelGGL((zn_aggregate_ell_kernel<A, BACKWARD, decltype(W)::value, decltype(NC)::value, decltype(MASK)::value, decltype(HEAD)::value>),
                               grid, dim3(GCN_THREADS), lds, s, a, geo.rows_per_block, geo.iters, partial);
        };
        // head: split 3 with ReLU + mask or without activation only, and the sign mask: ReLU at split 3 only (checked above)
        if constexpr (A == ACT_RELU) {
            if (a.head_in) return go(Const<2>{}, std::true_type{}, std::true_type{});
            if (a.mask) return go(Const<2>{}, std::true_type{}, std::false_type{});
        } else if constexpr (A == ACT_NONE) {
            if (a.head_in) return go(Const<2>{}, std::false_type{}, std::true_type{});
        }
        if (route == ELL_FAST3) go(Const<2>{}, std::false_type{}, std::false_type{});
        else go(Const<9>{}, std::false_type{}, std::false_type{});
    }); });
    return known ? finish_launch(BACKWARD, geo.blocks, a.c, partial, grad_bias, s) : GEOM_EINVAL;
}

// ---------------------------------------------------------------------------------------
// NARROW HEAD: the head layer when nobody reads its output beyond the three position columns (the last layer of a stack,
// geometrics_amd.layers._NarrowHead).  Only float4 group j = 0 of the aggregated slice reaches the positions, and in the
// backward only that group of the support gradient is non-zero, so both directions run thread (row, j = 0) of the fast
// kernel above and nothing else -- the same steps in the same order (table slots, then the CSR tail; term_load / term_add;
// Pack::bias_act), hence the same bits as the wide head's column group 0.  No [rows, c] tensor is written or read.
// ---------------------------------------------------------------------------------------
constexpr int NARROW_THREADS = 64; // forward: one row per lane, one wave per workgroup (the launch is a chain of three round trips)
constexpr int NARROW_PARTIAL_ROWS = 32; // rows per bias-gradient partial: the fast backward's rows_per_block * iters at k = 64

struct NarrowHeadArgs {
    const int *col;
    const float *val;
    const int *over_ptr, *over_col;
    const float *over_val;
    const float *support, *bias; // forward: [rows, c], [c] (may be null)
    const float *base;           // forward: [rows, 3]
    float *pos;                  // forward: [rows, 3]
    const float *grad_pos;       // backward: [rows, 3]
    unsigned short *sign;        // ReLU: one word per row, bit e <-> element e of the row's first float4 (null: no activation)
    float *gs;                   // backward: [rows, 4] = the support gradient's columns 0..3 (column 3 is zero)
    float *partial;              // backward: [meshes * chunks, c] column-sum partials, zero beyond column 2 (null: none)
    float scale;
    int nv, c, b, chunks;
};

template <int ACT, int W>
__global__ __launch_bounds__(NARROW_THREADS) void zn_narrow_head_fwd_kernel(NarrowHeadArgs a)
{
    int mesh_i, chunk_i;
    if (!geom::xcd_assign(blockIdx.x, a.b, a.chunks, mesh_i, chunk_i)) return;
    const int r = chunk_i * NARROW_THREADS + threadIdx.x;
    if (r >= a.nv) return;
    const int64_t mesh_row0 = (int64_t)mesh_i * a.nv, row = mesh_row0 + r;
    using KIND = TermKind<4, ACT, false>;
    const Source src{.x = a.support, .c = a.c};
    int nb[W];
    float w[W];
    load_table_row<W>(a.col, a.val, r, nb, w);
    int e0 = 0, e1 = 0;
    if (a.over_ptr) e0 = a.over_ptr[r], e1 = a.over_ptr[r + 1];
    Pack<4> sv[W], ov[W];
    unsigned nbits[W] = {};
    load_table_slots<KIND>(sv, ov, nbits, src, nb, mesh_row0, r, 0);
    Pack<4> acc = Pack<4>::zero();
    add_table_slots<KIND>(acc, sv, ov, nbits, nb, w);
    add_csr_run<KIND>(acc, src, a.over_col, a.over_val, e0, e1, mesh_row0, row, 0); // a row longer than the table
    acc.template bias_act<ACT, true>(a.bias, 0);
    if (ACT == ACT_RELU && a.sign) a.sign[row] = (unsigned short)acc.positive_bits();
    const float *bp = a.base + row * 3;
    float *pp = a.pos + row * 3;
#pragma unroll
    for (int e = 0; e < 3; ++e) pp[e] = bp[e] + a.scale * acc.at(e);
}

// One workgroup per bias-gradient partial of the wide head's backward: NARROW_PARTIAL_ROWS rows of one mesh, lane l < 32 owns
// row l.  The partial's three live columns are summed as the fast kernel sums them: thread rl of its 16 adds its two rows
// (tile 0, then tile 1) from zero, the sixteen sums are then added in rl order from zero.
template <int ACT, int W>
__global__ __launch_bounds__(NARROW_THREADS) void zn_narrow_head_bwd_kernel(NarrowHeadArgs a)
{
    __shared__ float4 own_lds[NARROW_PARTIAL_ROWS];
    int mesh_i, chunk_i;
    if (!geom::xcd_assign(blockIdx.x, a.b, a.chunks, mesh_i, chunk_i)) return;
    const int rl = threadIdx.x;
    const int r = chunk_i * NARROW_PARTIAL_ROWS + rl;
    const int64_t mesh_row0 = (int64_t)mesh_i * a.nv, row = mesh_row0 + r;
    using KIND = TermKind<4, ACT, true, ACT == ACT_RELU, true>;
    const Source src{.mask = a.sign, .kg = 1, .j = 0, .head = a.grad_pos, .head_scale = a.scale, .c = a.c};
    if (rl < NARROW_PARTIAL_ROWS) {
        Pack<4> own = Pack<4>::zero();
        if (r < a.nv) {
            int nb[W];
            float w[W];
            load_table_row<W>(a.col, a.val, r, nb, w);
            int e0 = 0, e1 = 0;
            if (a.over_ptr) e0 = a.over_ptr[r], e1 = a.over_ptr[r + 1];
            own_element<KIND>(own, src, row, 0);
            Pack<4> sv[W], ov[W];
            unsigned nbits[W] = {};
            load_table_slots<KIND>(sv, ov, nbits, src, nb, mesh_row0, r, 0);
            Pack<4> acc = Pack<4>::zero();
            add_table_slots<KIND>(acc, sv, ov, nbits, nb, w);
            add_csr_run<KIND>(acc, src, a.over_col, a.over_val, e0, e1, mesh_row0, row, 0);
            acc.store(a.gs + row * 4);
        }
        own_lds[rl] = own.v; // zeros for the rows beyond the mesh
    }
    if (!a.partial) return;
    __syncthreads();
    float *prow = a.partial + ((size_t)mesh_i * a.chunks + chunk_i) * a.c;
    for (int col = threadIdx.x; col < a.c; col += NARROW_THREADS) {
        float t = 0.f;
        if (col < 4) {
            constexpr int HALF = NARROW_PARTIAL_ROWS / 2;
            for (int l = 0; l < HALF; ++l) {
                float cs = 0.f;
                cs += elements(own_lds[l])[col];
                cs += elements(own_lds[l + HALF])[col];
                t += cs;
            }
        }
        prow[col] = t;
    }
}

template <bool BACKWARD>
int dispatch_narrow_head(NarrowHeadArgs a, int k, int w, int act, void *stream)
{
    if (const int code = check_sizes(a.b, a.nv, a.c, k)) return code;
    // the wide head's shapes (split 3, a table, ReLU with sign words or no activation) at the width whose backward partials are
    // NARROW_PARTIAL_ROWS rows each
    if (ell_route(a.c, k, w) != ELL_FAST3 || (act != ACT_RELU && act != ACT_NONE)) return GEOM_EUNSUPPORTED;
    const EllGeometry wide = ell_geometry(a.b > 0 ? a.b : 1, a.nv > 0 ? a.nv : 1, k, true);
    if (wide.rows_per_block * wide.iters != NARROW_PARTIAL_ROWS) return GEOM_EUNSUPPORTED;
    if (!BACKWARD && (!a.base || !a.pos)) return GEOM_EINVAL;
    if (BACKWARD && !a.grad_pos) return GEOM_EINVAL;
    if (a.b == 0 || a.nv == 0) return 0;
    if (!a.col || !a.val || (BACKWARD ? !a.gs : !a.support)) return GEOM_EINVAL;
    if (BACKWARD && act == ACT_RELU && !a.sign) return GEOM_EINVAL;
    if (act == ACT_NONE && a.sign) return GEOM_EINVAL;
    if (a.over_ptr && (!a.over_col || !a.over_val)) return GEOM_EINVAL;
    if ((((uintptr_t)a.col | (uintptr_t)a.val | (uintptr_t)a.support | (uintptr_t)a.bias | (uintptr_t)a.gs) % 16) != 0) return GEOM_EINVAL;
    if (a.b > 65535) return GEOM_ETOOBIG;
    a.chunks = BACKWARD ? wide.chunks : (a.nv + NARROW_THREADS - 1) / NARROW_THREADS;
    const dim3 grid(geom::xcd_grid(a.b, a.chunks));
    hipStream_t s = static_cast<hipStream_t>(stream);
    with_act(act, [&](auto ACT) { with_width(w, [&](auto W) {
        constexpr int A = decltype(ACT)::value == ACT_RELU ? ACT_RELU : ACT_NONE; // (ELU was refused above)
        if (BACKWARD) hipLaunchKernelGGL((zn_narrow_head_bwd_kernel<A, decltype(W)::value>), grid, dim3(NARROW_THREADS), 0, s, a);
        else hipLaunchKernelGGL((zn_narrow_head_fwd_kernel<A, decltype(W)::value>), grid, dim3(NARROW_THREADS), 0, s, a);
    }); });
    return geom::launch_status();
}

template <bool BACKWARD>
int dispatch(GcnArgs a, int b, int act, float *grad_bias, float *scratch, void *stream)
{
    if (const int code = check_sizes(b, a.nv, a.c, a.k)) return code;
    if (b == 0 || a.nv == 0 || a.c == 0) return 0;
    if (!a.rowptr || !a.x || !a.y || (a.k > 0 && (!a.col || !a.val))) return GEOM_EINVAL;
    if (const int code = check_gradient_operands<BACKWARD>(act, a.saved != nullptr, grad_bias, scratch)) return code;
    a.rows = (int64_t)b * a.nv;
    const bool vec4 = gcn_vec4(a.c, a.k);
    if (vec4 && (((uintptr_t)a.x | (uintptr_t)a.y | (uintptr_t)a.saved) % 16 != 0))
        return GEOM_EINVAL; // row-major fp32 tensors from any allocator are 16-byte aligned; refuse odd views
    if (!vec4 && a.c > GCN_THREADS) return GEOM_ETOOBIG;
    // (the mesh axis is checked in launch(), next to the block count)
    return vec4 ? launch<4, BACKWARD>(a, act, scratch, grad_bias, stream) : launch<1, BACKWARD>(a, act, scratch, grad_bias, stream);
}

} // namespace

extern "C" int geom_zn_gcn_aggregate_fwd_f32(int b, int nv, int c, int k, const int *rowptr, const int *col,
                                             const float *val, const float *support, const float *bias,
                                             int act, float *out, void *stream)
{
    GcnArgs a{rowptr, col, val, support, bias, nullptr, out, 0, nv, c, k};
    return dispatch<false>(a, b, act, nullptr, nullptr, stream);
}

extern "C" int64_t geom_zn_gcn_bwd_scratch_floats(int b, int nv, int c)
{
    if (b <= 0 || nv <= 0 || c <= 0) return 0;
    // upper bound over both vector widths (k is not known here): the scalar layout has fewer rows per block
    const int64_t b4 = (c % 4 == 0) ? gcn_geometry(b, nv, c, 4, true).blocks : 0;
    const int64_t b1 = gcn_geometry(b, nv, c, 1, true).blocks;
    return (b4 > b1 ? b4 : b1) * c;
}

// Rows of per-workgroup partial column sums the backward launches write into `scratch` for this shape: ell_w = the table
// width of the geom_zn_gcn_aggregate_ell_bwd_f32 call (8 / 16), 0 = geom_zn_gcn_aggregate_bwd_f32.  0: unsupported shape.
extern "C" int64_t geom_zn_gcn_bwd_partial_rows(int b, int nv, int c, int k, int ell_w)
{
    if (b <= 0 || nv <= 0 || c <= 0 || k < 0 || k > c) return 0;
    if (!ell_w) return gcn_geometry(b, nv, c, gcn_vec4(c, k) ? 4 : 1, true).blocks;
    const EllRoute route = ell_route(c, k, ell_w);
    if (route == ELL_ANY) return ell_any_geometry(b, nv, c, true).blocks;
    return route == ELL_NONE ? 0 : ell_geometry(b, nv, k, true).blocks;
}

extern "C" int geom_colsum_batch_f32(int count, const float *const *partials, const int *rows, const int *cols,
                                     float *const *outs, void *stream)
{
    if (count < 0 || count > GEOM_COLSUM_MAX_JOBS) return GEOM_ETOOBIG;
    if (count == 0) return 0;
    if (!partials || !rows || !cols || !outs) return GEOM_EINVAL;
    ColsumJobs jobs;
    int widest = 0;
    for (int i = 0; i < count; ++i) {
        if (!partials[i] || !outs[i] || rows[i] < 0 || cols[i] <= 0) return GEOM_EINVAL;
        jobs.partial[i] = partials[i], jobs.out[i] = outs[i], jobs.blocks[i] = rows[i], jobs.c[i] = cols[i];
        widest = cols[i] > widest ? cols[i] : widest;
    }
    hipLaunchKernelGGL(colsum_batch_kernel, dim3((widest + CS_COLS - 1) / CS_COLS, count), dim3(CS_COLS * CS_LANES), 0,
                       static_cast<hipStream_t>(stream), jobs);
    return geom::launch_status();
}

extern "C" int geom_zn_gcn_aggregate_bwd_f32(int b, int nv, int c, int k, const int *rowptrT, const int *colT,
                                             const float *valT, const float *grad_out, const float *out,
                                             int act, float *grad_support, float *grad_bias, float *scratch,
                                             void *stream)
{
    GcnArgs a{rowptrT, colT, valT, grad_out, nullptr, out, grad_support, 0, nv, c, k};
    return dispatch<true>(a, b, act, grad_bias, scratch, stream);
}

extern "C" int geom_zn_gcn_aggregate_ell_fwd_f32(int b, int nv, int c, int k, int w, const int *ell_col,
                                                 const float *ell_val, const int *over_ptr, const int *over_col,
                                                 const float *over_val, const float *support, const float *bias,
                                                 int act, float *out, uint16_t *relu_mask, void *stream)
{
    EllArgs a{.col = ell_col, .val = ell_val, .x = support, .bias = bias, .y = out, .nv = nv, .c = c, .k = k, .mask = relu_mask,
              .over_ptr = over_ptr, .over_col = over_col, .over_val = over_val};
    return dispatch_ell<false>(a, b, w, act, nullptr, nullptr, stream);
}

extern "C" int geom_zn_gcn_aggregate_ell_head_fwd_f32(int b, int nv, int c, int k, int w, const int *ell_col,
                                                      const float *ell_val, const int *over_ptr, const int *over_col,
                                                      const float *over_val, const float *support, const float *bias,
                                                      int act, float *out, uint16_t *relu_mask, const float *base,
                                                      float scale, float *pos, void *stream)
{
    if (!base || !pos) return GEOM_EINVAL;
    EllArgs a{.col = ell_col, .val = ell_val, .x = support, .bias = bias, .y = out, .nv = nv, .c = c, .k = k, .mask = relu_mask,
              .over_ptr = over_ptr, .over_col = over_col, .over_val = over_val, .head_in = base, .head_out = pos, .head_scale = scale};
    return dispatch_ell<false>(a, b, w, act, nullptr, nullptr, stream);
}

// Words of the ReLU sign mask: a property of the split alone, not of the route (either table width has the mask; beyond the fast
// kernel's 1024 aggregated columns the words are still counted, and the dispatcher refuses the mask).  0: no mask at this split.
extern "C" int64_t geom_zn_gcn_relu_mask_words(int b, int nv, int c, int k)
{
    if (b <= 0 || nv <= 0 || ell_nc(c, k) != 2) return 0;
    return (int64_t)b * nv * (k >> 2);
}

extern "C" int geom_zn_gcn_aggregate_ell_bwd_f32(int b, int nv, int c, int k, int w, const int *ell_colT,
                                                 const float *ell_valT, const int *over_ptrT, const int *over_colT,
                                                 const float *over_valT, const float *grad_out, const float *out,
                                                 const uint16_t *relu_mask, int act, float *grad_support,
                                                 float *grad_bias, float *scratch, void *stream)
{
    EllArgs a{.col = ell_colT, .val = ell_valT, .x = grad_out, .saved = out, .y = grad_support, .nv = nv, .c = c, .k = k,
              .mask = const_cast<uint16_t *>(relu_mask), .over_ptr = over_ptrT, .over_col = over_colT, .over_val = over_valT};
    return dispatch_ell<true>(a, b, w, act, grad_bias, scratch, stream);
}

extern "C" int geom_zn_gcn_aggregate_ell_head_bwd_f32(int b, int nv, int c, int k, int w, const int *ell_colT,
                                                      const float *ell_valT, const int *over_ptrT, const int *over_colT,
                                                      const float *over_valT, const float *grad_pos, float scale,
                                                      const uint16_t *relu_mask, int act, float *grad_support,
                                                      float *grad_bias, float *scratch, void *stream)
{
    if (!grad_pos) return GEOM_EINVAL;
    EllArgs a{.col = ell_colT, .val = ell_valT, .y = grad_support, .nv = nv, .c = c, .k = k, .mask = const_cast<uint16_t *>(relu_mask),
              .over_ptr = over_ptrT, .over_col = over_colT, .over_val = over_valT, .head_in = grad_pos, .head_scale = scale};
    return dispatch_ell<true>(a, b, w, act, grad_bias, scratch, stream);
}

extern "C" int geom_zn_gcn_narrow_head_fwd_f32(int b, int nv, int c, int k, int w, const int *ell_col, const float *ell_val,
                                               const int *over_ptr, const int *over_col, const float *over_val,
                                               const float *support, const float *bias, int act, const float *base,
                                               float scale, float *pos, uint16_t *sign_words, void *stream)
{
    NarrowHeadArgs a{.col = ell_col, .val = ell_val, .over_ptr = over_ptr, .over_col = over_col, .over_val = over_val,
                     .support = support, .bias = bias, .base = base, .pos = pos, .sign = sign_words, .scale = scale,
                     .nv = nv, .c = c, .b = b};
    return dispatch_narrow_head<false>(a, k, w, act, stream);
}

extern "C" int geom_zn_gcn_narrow_head_bwd_f32(int b, int nv, int c, int k, int w, const int *ell_colT, const float *ell_valT,
                                               const int *over_ptrT, const int *over_colT, const float *over_valT,
                                               const float *grad_pos, float scale, const uint16_t *sign_words, int act,
                                               float *grad_support4, float *partials, void *stream)
{
    NarrowHeadArgs a{.col = ell_colT, .val = ell_valT, .over_ptr = over_ptrT, .over_col = over_colT, .over_val = over_valT,
                     .grad_pos = grad_pos, .sign = const_cast<uint16_t *>(sign_words), .gs = grad_support4, .partial = partials,
                     .scale = scale, .nv = nv, .c = c, .b = b};
    return dispatch_narrow_head<true>(a, k, w, act, stream);
}
