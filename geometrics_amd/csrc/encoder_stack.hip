// The frozen mesh encoder's layers as ONE launch per layer and direction (reference models.py:386-435: sixteen BatchZERON_GCN
// layers 3 -> 60 ... -> 300 with ELU and a BatchGCNMax head), and the latent loss of the training step (GEOMetrics.py:165-171).
//
// A 0N-GCN layer aggregates only its first C / 10 columns -- at most 30 for every width of the encoder -- so they lie inside
// the first 32-deep k-stage of the NEXT layer's product: the tail of layer l (CSR gather + bias + ELU) is applied while that
// product's operand panel is staged, and nothing but the supports S_l ever travels between launches.  The mirror holds
// backward: g' = g * ELU'(X), [A^T . g'[:, :k] | g'[:, k:]] is the operand of the input-gradient product G . W^T.  With frozen
// parameters that is all a backward pass needs: no weight product, no split-K reduction, no column sums.
//
//   forward :  C[M][N] = T(S) . W,       T(S) = act([A . S[:, :k] | S[:, k:]] + bias),          W stored [K][N]
//   backward:  C[M][N] = T(g, X) . W^T,  T    = [A^T . g'[:, :k] | g'[:, k:]], g' = g * act'(X),  W stored [N][K]
//
// k = 0, no bias and act = NONE make T the identity (the first product positions . W_h1, K = 3); act = NONE with k > 0 is the
// adjoint tail of the head (no activation in front of its max).  The gather adds val * x in CSR order, un-fused, starting from
// 0.f: T equals geom_zn_gcn_aggregate_fwd_f32 / _bwd_f32 on the same input bit for bit (an optional pointer receives it, written
// by the workgroups of the first column tile).  The product is exact fp32 on v_mfma_f32_16x16x4_f32: the staged 64 x 64 tile of
// mfma_tiles.h with 32-deep stages -- the operand as [row][36], W as [k][68] in the forward and [row][36] in the backward (its
// panels, k permutation and lane map are stated there; dense_any.hip runs the same tile).  Workgroup = 64 x 64 tile, four waves 2 x 2; every global access is a
// bounds-checked 4-byte one (any M, N, K, pitch and alignment: 12-byte position rows, widths that are 2 mod 4), a wave reading
// 128-byte runs; the next stage's raw loads are in flight during a stage's MFMAs and are transformed when they are stored to the
// other LDS buffer: one barrier per stage.  A launch reads only what earlier launches wrote: no counters, no waiting.
#include "mfma_tiles.h"

namespace {

using namespace geom;

constexpr int ES_THREADS = 256;
constexpr int ES_T = TILE_N;    // tile edge (rows and columns)
constexpr int ES_BK = 32;       // stage depth: the aggregated columns (k <= 32) all lie in stage 0
constexpr int ES_PASSES = ES_T * ES_BK / ES_THREADS; // elements of a panel per thread

struct EncArgs {
    const int *rowptr, *col; // CSR (forward) / CSR^T (backward) of the adjacency the batch shares; unused when kagg == 0
    const float *val;
    const float *a;          // S (forward) / g (backward): [M][K], pitch lda
    const float *saved;      // backward: the layer's saved output X [M][K], pitch ldsaved (act != NONE)
    const float *bias;       // forward, may be null
    const float *w;          // forward [K][N], backward [N][K]; pitch ldw
    float *c;                // [M][N], pitch ldc
    float *t;                // the transformed operand [M][K], pitch ldt; may be null
    int64_t lda, ldsaved, ldw, ldc, ldt;
    int M, N, K, nv, kagg, tiles_n;
};

// what the epilogue of T does to a gathered / passed-through value
template <bool BWD, int ACT>
__device__ __forceinline__ float es_finish(float v, bool has_bias, float bias)
{
    if (BWD) return v;
    if (has_bias) v += bias; // (no bias: no addition -- a -0.f stays what it is, as in zn_gcn.hip)
    return act_fwd<ACT>(v);
}

// element (row, cc) of the operand in front of the gather: S, or g * act'(X)
template <bool BWD, int ACT>
__device__ __forceinline__ float es_source(const EncArgs &q, int64_t row, int cc)
{
    float v = q.a[row * q.lda + cc];
    if (BWD && ACT != ACT_NONE) v = act_bwd<ACT>(v, q.saved[row * q.ldsaved + cc]);
    return v;
}

template <bool BWD, int ACT>
__global__ __launch_bounds__(ES_THREADS) void encoder_layer_kernel(EncArgs q)
{
    constexpr int PK = tile_pk(ES_BK), PM = tile_pm(ES_T), PANEL = tile_panel(ES_T, ES_BK); // the panels of mfma_tiles.h
    __shared__ __attribute__((aligned(16))) float lds[4 * PANEL];
    float *const la = lds, *const lb = lds + 2 * PANEL;
    const int tid = threadIdx.x;
    const int nt = blockIdx.x % q.tiles_n, mt = blockIdx.x / q.tiles_n;
    const int m0 = mt * ES_T, n0 = nt * ES_T;
    const int nst = (q.K + ES_BK - 1) / ES_BK;
    const bool writes_t = q.t != nullptr && nt == 0;

    const int lane = tid & 63, wave = tid >> 6;
    const int x = lane & 15, g = lane >> 4;
    const int wr = tile_wave_row<2>(wave), wc = tile_wave_col(wave);

    // operand panel: thread -> column kk of the stage, rows r0 + 8 p (a wave reads two 128-byte runs per pass)
    const int a_kk = tid & 31, a_r0 = tid >> 5;
    // weight panel: forward [k][n] -> k = w_r0 + 4 p, n = tid & 63; backward [n][k] -> n = a_r0 + 8 p, k = a_kk
    const int w_n = tid & 63, w_r0 = tid >> 6;

    float ra[ES_PASSES], rs[ES_PASSES], rw[ES_PASSES];
    float rbias = 0.f;

    auto load_raw = [&](int st) {
        const int cc = st * ES_BK + a_kk;
        const bool kin = cc < q.K;
        if (!BWD) rbias = (kin && q.bias) ? q.bias[cc] : 0.f;
#pragma unroll
        for (int p = 0; p < ES_PASSES; ++p) {
            const int64_t row = m0 + a_r0 + 8 * p;
            const bool in = kin && row < q.M;
            ra[p] = in ? q.a[row * q.lda + cc] : 0.f;
            if (BWD && ACT != ACT_NONE) rs[p] = in ? q.saved[row * q.ldsaved + cc] : 0.f;
        }
    };
    auto load_w = [&](int st) {
#pragma unroll
        for (int p = 0; p < ES_PASSES; ++p) {
            if (!BWD) {
                const int kk = st * ES_BK + w_r0 + 4 * p, n = n0 + w_n;
                rw[p] = (kk < q.K && n < q.N) ? q.w[(int64_t)kk * q.ldw + n] : 0.f;
            } else {
                const int kk = st * ES_BK + a_kk, n = n0 + a_r0 + 8 * p;
                rw[p] = (kk < q.K && n < q.N) ? q.w[(int64_t)n * q.ldw + kk] : 0.f;
            }
        }
    };
    // stages >= 1 (no aggregated columns): transform the raw loads and store both panels
    auto store_stage = [&](int st, float *as, float *bs) {
        const int cc = st * ES_BK + a_kk;
#pragma unroll
        for (int p = 0; p < ES_PASSES; ++p) {
            const int r = a_r0 + 8 * p;
            const int64_t row = m0 + r;
            const bool in = cc < q.K && row < q.M;
            float v = ra[p];
            if (BWD && ACT != ACT_NONE) v = act_bwd<ACT>(v, rs[p]);
            v = in ? es_finish<BWD, ACT>(v, q.bias != nullptr, rbias) : 0.f;
            as[r * PK + a_kk] = v;
            if (writes_t && in) q.t[row * q.ldt + cc] = v;
        }
#pragma unroll
        for (int p = 0; p < ES_PASSES; ++p) {
            if (!BWD) bs[(w_r0 + 4 * p) * PM + w_n] = rw[p];
            else bs[(a_r0 + 8 * p) * PK + a_kk] = rw[p];
        }
    };

    f32x4 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

    auto compute = [&](const float *as, const float *bs) { tile_stage<false, !BWD, 2, ES_BK>(as, bs, wr, wc, x, g, acc); };

    if (nst > 0) {
        // ---- stage 0: the columns below kagg are gathered over the row's CSR entries, in CSR order, starting from 0.f
        load_w(0);
        const int cc = a_kk;
        const bool kin = cc < q.K;
        const float bias0 = (!BWD && kin && q.bias) ? q.bias[cc] : 0.f;
        float v0[ES_PASSES];
        if (kin && cc < q.kagg) {
            // the thread's eight rows side by side, NB entries of each per round: a round is two round trips (entries, then the
            // neighbours' elements) whatever the rows' lengths; the sum of a row stays in CSR order (rounds, then slots, ascending)
            constexpr int NB = (BWD && ACT != ACT_NONE) ? 2 : 4;
            int e0[ES_PASSES], e1[ES_PASSES], base[ES_PASSES];
            int longest = 0;
#pragma unroll
            for (int p = 0; p < ES_PASSES; ++p) {
                const int row = m0 + a_r0 + 8 * p;
                const bool live = row < q.M;
                base[p] = live ? row / q.nv * q.nv : 0;
                e0[p] = live ? q.rowptr[row - base[p]] : 0;
                e1[p] = live ? q.rowptr[row - base[p] + 1] : 0;
                longest = max(longest, e1[p] - e0[p]);
                v0[p] = 0.f;
            }
            for (int off = 0; off < longest; off += NB) {
                int cj[ES_PASSES][NB];
                float wj[ES_PASSES][NB], sj[ES_PASSES][NB], oj[ES_PASSES][NB];
#pragma unroll
                for (int p = 0; p < ES_PASSES; ++p)
#pragma unroll
                    for (int j = 0; j < NB; ++j) {
                        const int e = e0[p] + off + j;
                        const bool live = e < e1[p];
                        cj[p][j] = live ? q.col[e] : -1;
                        wj[p][j] = live ? q.val[e] : 0.f;
                    }
#pragma unroll
                for (int p = 0; p < ES_PASSES; ++p)
#pragma unroll
                    for (int j = 0; j < NB; ++j) {
                        const bool live = cj[p][j] >= 0;
                        const int64_t nb = (int64_t)base[p] + (live ? cj[p][j] : 0);
                        sj[p][j] = live ? q.a[nb * q.lda + cc] : 0.f;
                        oj[p][j] = (live && BWD && ACT != ACT_NONE) ? q.saved[nb * q.ldsaved + cc] : 0.f;
                    }
#pragma unroll
                for (int p = 0; p < ES_PASSES; ++p)
#pragma unroll
                    for (int j = 0; j < NB; ++j)
                        if (cj[p][j] >= 0) {
                            float sv = sj[p][j];
                            if (BWD && ACT != ACT_NONE) sv = act_bwd<ACT>(sv, oj[p][j]);
                            v0[p] += wj[p][j] * sv;
                        }
            }
        } else {
#pragma unroll
            for (int p = 0; p < ES_PASSES; ++p) {
                const int64_t row = m0 + a_r0 + 8 * p;
                v0[p] = (kin && row < q.M) ? es_source<BWD, ACT>(q, row, cc) : 0.f;
            }
        }
#pragma unroll
        for (int p = 0; p < ES_PASSES; ++p) {
            const int r = a_r0 + 8 * p;
            const int64_t row = m0 + r;
            const bool in = kin && row < q.M;
            const float v = in ? es_finish<BWD, ACT>(v0[p], q.bias != nullptr, bias0) : 0.f;
            if (writes_t && in) q.t[row * q.ldt + cc] = v;
            la[r * PK + a_kk] = v;
        }
#pragma unroll
        for (int p = 0; p < ES_PASSES; ++p) {
            if (!BWD) lb[(w_r0 + 4 * p) * PM + w_n] = rw[p];
            else lb[(a_r0 + 8 * p) * PK + a_kk] = rw[p];
        }
        __syncthreads();
    }
    for (int st = 0; st < nst; ++st) {
        const int cur = st & 1;
        if (st + 1 < nst) {
            load_raw(st + 1);
            load_w(st + 1);
        }
        compute(la + cur * PANEL, lb + cur * PANEL);
        if (st + 1 < nst) store_stage(st + 1, la + (cur ^ 1) * PANEL, lb + (cur ^ 1) * PANEL);
        __syncthreads();
    }

    tile_for_each_output<2>(acc, m0 + wr, n0 + wc, x, g, [&](int m, int n, const f32x4 &v) {
        if (m < q.M) {
            float *o = q.c + (int64_t)m * q.ldc + n;
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (n + r < q.N) o[r] = v[r];
        }
    });
}

template <bool BWD>
void encoder_launch(const EncArgs &q, int act, dim3 grid, hipStream_t s)
{
    if (act == ACT_ELU) hipLaunchKernelGGL((encoder_layer_kernel<BWD, ACT_ELU>), grid, dim3(ES_THREADS), 0, s, q);
    else if (act == ACT_RELU) hipLaunchKernelGGL((encoder_layer_kernel<BWD, ACT_RELU>), grid, dim3(ES_THREADS), 0, s, q);
    else hipLaunchKernelGGL((encoder_layer_kernel<BWD, ACT_NONE>), grid, dim3(ES_THREADS), 0, s, q);
}

// the size checks shared by the two directions, in front of any pointer check
int encoder_check(int b, int nv, int c, int k, int n, int act)
{
    if (b < 0 || nv < 0 || c < 0 || k < 0 || n < 0 || k > c) return GEOM_EINVAL;
    if (act < ACT_NONE || act > ACT_ELU) return GEOM_EINVAL;
    if (k > ES_BK) return GEOM_EUNSUPPORTED; // the aggregated columns must lie inside the first k-stage
    if ((int64_t)b * nv > 0x7fffffffLL - ES_T) return GEOM_ETOOBIG;
    return 0;
}

int encoder_run(bool bwd, EncArgs &q, int act, hipStream_t s)
{
    if (q.K == 0) // an empty sum
        return (int)hipMemset2DAsync(q.c, (size_t)q.ldc * 4, 0, (size_t)q.N * 4, (size_t)q.M, s) ? GEOM_EINVAL : 0;
    q.tiles_n = (q.N + ES_T - 1) / ES_T;
    const int64_t blocks = (int64_t)((q.M + ES_T - 1) / ES_T) * q.tiles_n;
    if (blocks > 0x7fffffffLL) return GEOM_ETOOBIG;
    if (bwd) encoder_launch<true>(q, act, dim3((unsigned)blocks), s);
    else encoder_launch<false>(q, act, dim3((unsigned)blocks), s);
    return geom::launch_status();
}

// ---- latent loss: w * sum_b [ mean_j |pred[b][j] - target[b][j]| * on[b] / sum(on) ]  (GEOMetrics.py:167) -----------------
// One workgroup; every sum in a fixed order (thread t owns meshes t, t + 256, ...; the 256 thread sums are added in ascending
// order).  sum(on) == 0 gives 0 -- decided here, not on the host.
constexpr int LL_THREADS = 256;

__device__ __forceinline__ float ll_block_sum(float v, float *sh)
{
    sh[threadIdx.x] = v;
    __syncthreads();
    float t = 0.f;
    for (int i = 0; i < LL_THREADS; ++i) t += sh[i];
    __syncthreads();
    return t;
}

__global__ __launch_bounds__(LL_THREADS) void latent_l1_fwd_kernel(int b, int l, const float *__restrict__ pred,
                                                                   const float *__restrict__ target, const float *__restrict__ on,
                                                                   float weight, float *__restrict__ loss)
{
    __shared__ float sh[LL_THREADS];
    float part = 0.f;
    for (int m = threadIdx.x; m < b; m += LL_THREADS) part += on[m];
    const float total = ll_block_sum(part, sh);
    float mine = 0.f;
    if (total != 0.f) {
        for (int m = threadIdx.x; m < b; m += LL_THREADS) {
            float sum = 0.f;
            for (int j = 0; j < l; ++j) sum += fabsf(pred[(int64_t)m * l + j] - target[(int64_t)m * l + j]);
            mine += sum / (float)l * on[m] / total;
        }
    }
    const float all = ll_block_sum(mine, sh);
    if (threadIdx.x == 0) loss[0] = total != 0.f ? weight * all : 0.f;
}

__global__ __launch_bounds__(LL_THREADS) void latent_l1_bwd_kernel(int b, int l, const float *__restrict__ pred,
                                                                   const float *__restrict__ target, const float *__restrict__ on,
                                                                   float weight, const float *__restrict__ grad_loss,
                                                                   float *__restrict__ grad_pred)
{
    __shared__ float sh[LL_THREADS];
    float part = 0.f;
    for (int m = threadIdx.x; m < b; m += LL_THREADS) part += on[m];
    const float total = ll_block_sum(part, sh);
    const int64_t count = (int64_t)b * l;
    const float go = grad_loss[0];
    for (int64_t e = (int64_t)blockIdx.x * LL_THREADS + threadIdx.x; e < count; e += (int64_t)gridDim.x * LL_THREADS) {
        float gr = 0.f;
        if (total != 0.f) {
            const float d = pred[e] - target[e];
            const float sign = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);
            gr = go * weight * (on[e / l] / total) / (float)l * sign;
        }
        grad_pred[e] = gr;
    }
}

} // namespace

extern "C" int geom_encoder_layer_fwd_f32(int b, int nv, int c, int k, int n, const int *rowptr, const int *col, const float *val,
                                          const float *s, int64_t lds, const float *bias, int act, const float *w, int64_t ldw,
                                          float *out, int64_t ldo, float *x_out, int64_t ldx, void *stream)
{
    const int bad = encoder_check(b, nv, c, k, n, act);
    if (bad) return bad;
    if ((int64_t)b * nv == 0 || n == 0) return 0;
    if (!out || ldo < n) return GEOM_EINVAL;
    if (c > 0 && (!s || !w || lds < c || ldw < n)) return GEOM_EINVAL;
    if (k > 0 && (!rowptr || !col || !val)) return GEOM_EINVAL;
    if (x_out && ldx < c) return GEOM_EINVAL;
    EncArgs q;
    q.rowptr = rowptr, q.col = col, q.val = val, q.a = s, q.saved = nullptr, q.bias = bias, q.w = w, q.c = out, q.t = x_out;
    q.lda = lds, q.ldsaved = 0, q.ldw = ldw, q.ldc = ldo, q.ldt = ldx;
    q.M = b * nv, q.N = n, q.K = c, q.nv = nv, q.kagg = k, q.tiles_n = 0;
    return encoder_run(false, q, act, static_cast<hipStream_t>(stream));
}

extern "C" int geom_encoder_layer_bwd_f32(int b, int nv, int c, int k, int n, const int *rowptrT, const int *colT, const float *valT,
                                          const float *g, int64_t ldg, const float *x_saved, int64_t ldx, int act, const float *w,
                                          int64_t ldw, float *out, int64_t ldo, float *t_out, int64_t ldt, void *stream)
{
    const int bad = encoder_check(b, nv, c, k, n, act);
    if (bad) return bad;
    if ((int64_t)b * nv == 0 || n == 0) return 0;
    if (!out || ldo < n) return GEOM_EINVAL;
    if (c > 0 && (!g || !w || ldg < c || ldw < c)) return GEOM_EINVAL;
    if (c > 0 && act != ACT_NONE && (!x_saved || ldx < c)) return GEOM_EINVAL;
    if (k > 0 && (!rowptrT || !colT || !valT)) return GEOM_EINVAL;
    if (t_out && ldt < c) return GEOM_EINVAL;
    EncArgs q;
    q.rowptr = rowptrT, q.col = colT, q.val = valT, q.a = g, q.saved = x_saved, q.bias = nullptr, q.w = w, q.c = out, q.t = t_out;
    q.lda = ldg, q.ldsaved = ldx, q.ldw = ldw, q.ldc = ldo, q.ldt = ldt;
    q.M = b * nv, q.N = n, q.K = c, q.nv = nv, q.kagg = k, q.tiles_n = 0;
    return encoder_run(true, q, act, static_cast<hipStream_t>(stream));
}

extern "C" int geom_latent_l1_fwd_f32(int b, int l, const float *pred, const float *target, const float *on, float weight, float *loss,
                                      void *stream)
{
    if (b < 0 || l < 0) return GEOM_EINVAL;
    if (!loss) return GEOM_EINVAL;
    if ((int64_t)b * l > 0 && (!pred || !target || !on)) return GEOM_EINVAL;
    if (l == 0) b = 0; // no elements: sum(on) is not read, the loss is 0
    hipLaunchKernelGGL(latent_l1_fwd_kernel, dim3(1), dim3(LL_THREADS), 0, static_cast<hipStream_t>(stream), b, l, pred, target, on,
                       weight, loss);
    return geom::launch_status();
}

extern "C" int geom_latent_l1_bwd_f32(int b, int l, const float *pred, const float *target, const float *on, float weight,
                                      const float *grad_loss, float *grad_pred, void *stream)
{
    if (b < 0 || l < 0) return GEOM_EINVAL;
    const int64_t count = (int64_t)b * l;
    if (count == 0) return 0;
    if (!pred || !target || !on || !grad_loss || !grad_pred) return GEOM_EINVAL;
    int64_t blocks = (count + LL_THREADS - 1) / LL_THREADS;
    if (blocks > 1024) blocks = 1024;
    hipLaunchKernelGGL(latent_l1_bwd_kernel, dim3((unsigned)blocks), dim3(LL_THREADS), 0, static_cast<hipStream_t>(stream), b, l, pred,
                       target, on, weight, grad_loss, grad_pred);
    return geom::launch_status();
}
