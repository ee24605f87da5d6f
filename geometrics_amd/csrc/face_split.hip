// Adaptive face splitting (old_GEOMetrics/utils.py:431-634: calc_curve, split_info) on the device.
//
// The reference measures every active face's mean dihedral angle to its three neighbours with ~20 eager ops, then splits the
// faces above a threshold in ~150 lines of numpy on the host: a dense (V+S)^2 float64 matrix per call and several
// device -> host -> device round trips, twice per mesh and step (old_GEOMetrics/GEOMetrics.py:105-118, 185-191).  Here:
//
//   geom_face_curvature_f32       one launch, a thread per active face: its own and its three neighbours' normals are recomputed
//                                 in registers (no normals pass), in the reference's arithmetic and order;
//   geom_face_select_f32          one workgroup: flag, ordered compaction, count and the three largest curvatures;
//   geom_face_split_index         one workgroup: the index tables of a split (where each split row and face stands in the list, the
//                                 unsplit rows' ranks, the vertex -> split-face incidence in ascending order), no host read;
//   geom_face_split_tables        one launch over three row ranges: the new `faces` rows, the new `face_list` rows and the rows of
//                                 the new adjacency -- CSR (its transpose has the same pattern) with the values of the normalised
//                                 matrix in both orientations, and the non-zeros of the two dense matrices;
//   geom_split_vertices_fwd_f32   old rows copied, new rows (x/3 + y/3) + z/3 with true divisions;
//   geom_split_vertices_bwd_f32   the transpose as a gather over the vertex -> split-face incidence table: no atomics.
// For the union of a ragged batch (one mesh to the launches above, except the two that are one workgroup by design):
//   geom_face_select_ragged_f32   two launches of a workgroup per mesh: each mesh's own count, fallback and place in the list;
//   geom_face_split_index_ragged  the same index tables and the new mesh ids from four launches over chunks of 256 items and
//                                 one zero-fill, no workgroup waiting on another.
//
// Every index a kernel follows is checked against the size of what it points into before it is used: a table that names a row
// outside leaves a NaN (floats) or the raw value (indices) instead of reading or writing out of bounds.
#include "geom_common.h"

namespace {

constexpr int SPLIT_THREADS = 256;

// ---------------------------------------------------------------------------------------------------- curvature ----
// face normal in the reference's order (utils.py:437-446): p1 = v[f[1]], p2 = v[f[0]], p3 = v[f[2]], cross(p2 - p1, p3 - p1) / |.|
__device__ __forceinline__ bool face_normal(const float *verts, int nv, const int64_t *faces, int64_t nft, int64_t f, float n[3])
{
    if (f < 0 || f >= nft) return false;
    const int64_t i0 = faces[3 * f], i1 = faces[3 * f + 1], i2 = faces[3 * f + 2];
    if (i0 < 0 || i0 >= nv || i1 < 0 || i1 >= nv || i2 < 0 || i2 >= nv) return false;
    const float *p1 = verts + 3 * i1, *p2 = verts + 3 * i0, *p3 = verts + 3 * i2;
    const float ax = p2[0] - p1[0], ay = p2[1] - p1[1], az = p2[2] - p1[2];
    const float bx = p3[0] - p1[0], by = p3[1] - p1[1], bz = p3[2] - p1[2];
    const float cx = ay * bz - az * by, cy = az * bx - ax * bz, cz = ax * by - ay * bx;
    const float q = sqrtf((cx * cx + cy * cy) + cz * cz);
    n[0] = cx / q, n[1] = cy / q, n[2] = cz / q;
    return true;
}

__global__ __launch_bounds__(SPLIT_THREADS) void face_curvature_kernel(int nv, const float *verts, int nft, const int64_t *faces,
                                                                       int nfa, const int64_t *face_list, float *curv)
{
    const int i = blockIdx.x * SPLIT_THREADS + threadIdx.x;
    if (i >= nfa) return;
    const int64_t *row = face_list + 9 * (int64_t)i;
    const float eps = .00001f;
    float own[3], nb[3];
    bool ok = face_normal(verts, nv, faces, nft, row[2], own);
    float sum = 0.f;
    for (int j = 0; j < 3 && ok; ++j) {
        ok = face_normal(verts, nv, faces, nft, row[3 * j], nb);
        if (!ok) break;
        float d = (own[0] * nb[0] + own[1] * nb[1]) + own[2] * nb[2];
        d = d < -1.0f + eps ? -1.0f + eps : (d > 1.0f - eps ? 1.0f - eps : d); // NaN passes through both comparisons
        sum += acosf(d);
    }
    curv[i] = ok ? sum / 3.0f : __builtin_nanf("");
}

// ---------------------------------------------------------------------------------------------------- selection ----
// "is (va, ia) ahead of (vb, ib)" in the order of the fallback: larger curvature first, lower position on ties; NaN never ahead
__device__ __forceinline__ bool ahead(float va, int ia, float vb, int ib)
{
    if (ia < 0) return false;
    if (ib < 0) return true;
    return va > vb || (va == vb && ia < ib);
}

__device__ __forceinline__ void top3_insert(float v, int i, float tv[3], int ti[3])
{
    if (v != v) return; // a degenerate face is never selected
    for (int k = 0; k < 3; ++k)
        if (ahead(v, i, tv[k], ti[k])) {
            for (int m = 2; m > k; --m) tv[m] = tv[m - 1], ti[m] = ti[m - 1];
            tv[k] = v, ti[k] = i;
            return;
        }
}

// One workgroup; thread t owns the contiguous chunk [t * per, (t + 1) * per) of the active list, so the compaction is ordered.
// out[0] = number of faces with (c * 180) / pi > angle, out[1..3] = the positions of the three largest curvatures (-1: fewer
// than three faces with a curvature); selected[0 .. out[0]) = the flagged positions, ascending.
__global__ __launch_bounds__(SPLIT_THREADS) void face_select_kernel(int nfa, const float *curv, float angle, int64_t *selected,
                                                                    int64_t *out)
{
    __shared__ int counts[SPLIT_THREADS];
    __shared__ float cand_v[3 * SPLIT_THREADS];
    __shared__ int cand_i[3 * SPLIT_THREADS];
    const int t = threadIdx.x;
    const int per = (nfa + SPLIT_THREADS - 1) / SPLIT_THREADS;
    const int lo = t * per < nfa ? t * per : nfa, hi = lo + per < nfa ? lo + per : nfa;
    const float pi = 3.14159265358979323846f;
    float tv[3] = {0.f, 0.f, 0.f};
    int ti[3] = {-1, -1, -1};
    int n = 0;
    for (int i = lo; i < hi; ++i) {
        const float c = curv[i];
        n += ((c * 180.0f) / pi > angle) ? 1 : 0;
        top3_insert(c, i, tv, ti);
    }
    counts[t] = n;
    for (int k = 0; k < 3; ++k) cand_v[3 * t + k] = tv[k], cand_i[3 * t + k] = ti[k];
    __syncthreads();
    if (t == 0) { // 256 counts and 768 candidates: a serial pass, in a fixed order
        int run = 0;
        for (int k = 0; k < SPLIT_THREADS; ++k) {
            const int c = counts[k];
            counts[k] = run;
            run += c;
        }
        float bv[3] = {0.f, 0.f, 0.f};
        int bi[3] = {-1, -1, -1};
        for (int k = 0; k < 3 * SPLIT_THREADS; ++k)
            if (cand_i[k] >= 0) top3_insert(cand_v[k], cand_i[k], bv, bi);
        out[0] = run;
        for (int k = 0; k < 3; ++k) out[1 + k] = bi[k];
    }
    __syncthreads();
    int at = counts[t];
    for (int i = lo; i < hi; ++i) {
        const float c = curv[i];
        if ((c * 180.0f) / pi > angle) selected[at++] = i;
    }
}

// -------------------------------------------------------------------------------------------------- index tables ----
struct SplitIndexArgs {
    int nv, nft, nfa, s;
    const int64_t *faces, *face_list, *splitting;
    int64_t *corners, *split_pos, *unsplit_rank, *face_s, *inc_ptr, *inc_item, *cursor;
};

// exclusive prefix of `mine` over the threads of the workgroup, in thread order (256 values: a serial pass by thread 0)
__device__ __forceinline__ int block_offset(int mine, int *lds)
{
    __syncthreads(); // lds may still be read from a previous call
    lds[threadIdx.x] = mine;
    __syncthreads();
    if (threadIdx.x == 0) {
        int run = 0;
        for (int k = 0; k < SPLIT_THREADS; ++k) {
            const int c = lds[k];
            lds[k] = run;
            run += c;
        }
    }
    __syncthreads();
    return lds[threadIdx.x];
}

// One workgroup makes every index table of a split (the tables are small and the steps depend on each other: scatter, running
// sums, ordered fill).  The incidence rows are filled through a per-vertex cursor in arrival order and then sorted in place by
// the vertex's thread (a row is as long as the vertex has split faces: at most its degree), so the result does not depend on
// the order the atomics were served in.
__global__ __launch_bounds__(SPLIT_THREADS) void face_split_index_kernel(SplitIndexArgs a)
{
    __shared__ int lds[SPLIT_THREADS];
    const int t = threadIdx.x;
    for (int i = t; i < a.nfa; i += SPLIT_THREADS) a.split_pos[i] = -1;
    for (int i = t; i < a.nft; i += SPLIT_THREADS) a.face_s[i] = -1;
    for (int i = t; i <= a.nv; i += SPLIT_THREADS) a.inc_ptr[i] = 0;
    for (int i = t; i < a.nv; i += SPLIT_THREADS) a.cursor[i] = 0;
    for (int64_t i = t; i < 3 * (int64_t)a.s; i += SPLIT_THREADS) a.inc_item[i] = -1;
    __syncthreads();
    for (int k = t; k < a.s; k += SPLIT_THREADS) { // scatter: where each split row / face stands in `splitting`; corner counts
        const int64_t p = a.splitting[k];
        int64_t c[3] = {-1, -1, -1};
        if (p >= 0 && p < a.nfa) {
            a.split_pos[p] = k;
            const int64_t own = a.face_list[9 * p + 2];
            if (own >= 0 && own < a.nft) {
                a.face_s[own] = k;
                for (int j = 0; j < 3; ++j) c[j] = a.faces[3 * own + j];
            }
        }
        for (int j = 0; j < 3; ++j) {
            a.corners[3 * (int64_t)k + j] = c[j];
            if (c[j] >= 0 && c[j] < a.nv) atomicAdd(reinterpret_cast<unsigned long long *>(a.inc_ptr + c[j] + 1), 1ull);
        }
    }
    __syncthreads();
    { // unsplit_rank[i] = how many unsplit rows precede row i: a contiguous chunk per thread
        const int per = (a.nfa + SPLIT_THREADS - 1) / SPLIT_THREADS;
        const int lo = t * per < a.nfa ? t * per : a.nfa, hi = lo + per < a.nfa ? lo + per : a.nfa;
        int n = 0;
        for (int i = lo; i < hi; ++i) n += a.split_pos[i] < 0 ? 1 : 0;
        int64_t at = block_offset(n, lds);
        for (int i = lo; i < hi; ++i) {
            a.unsplit_rank[i] = at;
            at += a.split_pos[i] < 0 ? 1 : 0;
        }
    }
    { // inc_ptr[u + 1] holds vertex u's count: running sum in place
        const int per = (a.nv + SPLIT_THREADS - 1) / SPLIT_THREADS;
        const int lo = t * per < a.nv ? t * per : a.nv, hi = lo + per < a.nv ? lo + per : a.nv;
        // (the counts were made by atomics, which are served in L2: they are read there, not through the CU's cache)
        int n = 0;
        for (int u = lo; u < hi; ++u) n += (int)__hip_atomic_load(a.inc_ptr + u + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        int64_t at = block_offset(n, lds);
        for (int u = lo; u < hi; ++u) {
            at += __hip_atomic_load(a.inc_ptr + u + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            a.inc_ptr[u + 1] = at;
        }
    }
    __syncthreads();
    for (int k = t; k < a.s; k += SPLIT_THREADS)
        for (int j = 0; j < 3; ++j) {
            const int64_t c = a.corners[3 * (int64_t)k + j];
            if (c < 0 || c >= a.nv) continue;
            const int64_t at = a.inc_ptr[c] + (int64_t)atomicAdd(reinterpret_cast<unsigned long long *>(a.cursor + c), 1ull);
            if (at < a.inc_ptr[c + 1] && at < 3 * (int64_t)a.s) a.inc_item[at] = k;
        }
    __syncthreads();
    for (int u = t; u < a.nv; u += SPLIT_THREADS) { // ascending split order within every vertex's row
        const int64_t lo = a.inc_ptr[u], hi = a.inc_ptr[u + 1];
        if (lo < 0 || hi > 3 * (int64_t)a.s) continue;
        for (int64_t i = lo + 1; i < hi; ++i) {
            const int64_t v = a.inc_item[i];
            int64_t j = i;
            for (; j > lo && a.inc_item[j - 1] > v; --j) a.inc_item[j] = a.inc_item[j - 1];
            a.inc_item[j] = v;
        }
    }
}

// ------------------------------------------------------------------------------------------------------- tables ----
__device__ __forceinline__ int new_row_length(const geom_face_split &a, int w)
{
    if (w >= a.nv) return 4; // a new vertex: its three corners and itself
    return (a.rowptr[w + 1] - a.rowptr[w]) + (int)(a.inc_ptr[w + 1] - a.inc_ptr[w]);
}

// entry `at` of the new CSR, row r -> column w, and the same element of the two dense matrices
__device__ __forceinline__ void put_entry(const geom_face_split &a, int64_t at, int r, int64_t w, float inv_len)
{
    const int n = a.nv + a.s;
    if (at < 0 || at >= (int64_t)a.nnz + 7 * (int64_t)a.s || w < 0 || w >= n) return;
    a.new_col[at] = (int)w;
    a.new_val[at] = inv_len;
    a.new_val_t[at] = 1.0f / (float)new_row_length(a, (int)w);
    a.new_ones[at] = 1.0f;
    if (a.adj) a.adj[(size_t)r * n + w] = inv_len;
    if (a.adj_orig) a.adj_orig[(size_t)r * n + w] = 1.0f;
}

// where face f stands after the split, seen across the edge its neighbour labels `label` (the reference's new_positions,
// utils.py:509-511): a split face is replaced by its child that kept that edge
__device__ __forceinline__ int64_t new_position(const geom_face_split &a, int64_t f, int64_t label)
{
    if (f < 0 || f >= a.nft || label < 0 || label > 2) return f;
    const int64_t s = a.face_s[f];
    return (s >= 0 && s < a.s) ? a.nft + label * a.s + s : f;
}

__device__ __forceinline__ void put_slot(int64_t *row, int slot, int64_t face, int64_t label, int64_t own)
{
    row[3 * slot] = face, row[3 * slot + 1] = label, row[3 * slot + 2] = own;
}

__global__ __launch_bounds__(SPLIT_THREADS) void face_split_tables_kernel(geom_face_split a)
{
    const int64_t n_face_rows = (int64_t)a.nft + 3 * (int64_t)a.s, n_rows = (int64_t)a.nv + a.s;
    int64_t id = (int64_t)blockIdx.x * SPLIT_THREADS + threadIdx.x;
    if (id < n_face_rows) { // ---- `faces`: old rows stay (dead where split), then the S first, second and third children
        int64_t x, y, z;
        if (id < a.nft) {
            x = a.faces[3 * id], y = a.faces[3 * id + 1], z = a.faces[3 * id + 2];
        } else {
            const int64_t k = (id - a.nft) / a.s, s = (id - a.nft) - k * a.s, nw = a.nv + s;
            x = a.corners[3 * s], y = a.corners[3 * s + 1], z = a.corners[3 * s + 2];
            if (k == 0) z = nw;
            else if (k == 1) x = nw;
            else y = nw;
        }
        a.new_faces[3 * id] = x, a.new_faces[3 * id + 1] = y, a.new_faces[3 * id + 2] = z;
        return;
    }
    id -= n_face_rows;
    if (id < a.nfa) { // ---- `face_list`: a thread per OLD active row writes that row, or its three children's rows
        const int64_t *row = a.face_list + 9 * id;
        const int64_t unsplit = (int64_t)a.nfa - a.s, rows_out = (int64_t)a.nfa + 2 * (int64_t)a.s;
        int64_t across[3];
        for (int j = 0; j < 3; ++j) across[j] = new_position(a, row[3 * j], row[3 * j + 1]);
        const int64_t s = a.split_pos[id];
        if (s < 0 || s >= a.s) {
            const int64_t q = a.unsplit_rank[id];
            if (q < 0 || q >= unsplit) return;
            for (int j = 0; j < 3; ++j) put_slot(a.new_face_list + 9 * q, j, across[j], row[3 * j + 1], row[2]);
            return;
        }
        const int64_t c1 = a.nft + s, c2 = c1 + a.s, c3 = c2 + a.s;
        int64_t *o1 = a.new_face_list + 9 * (unsplit + s), *o2 = o1 + 9 * (int64_t)a.s, *o3 = o2 + 9 * (int64_t)a.s;
        if (unsplit + 2 * (int64_t)a.s + s >= rows_out) return;
        put_slot(o1, 0, across[0], row[1], c1), put_slot(o1, 1, c2, 0, c1), put_slot(o1, 2, c3, 0, c1);
        put_slot(o2, 0, c1, 1, c2), put_slot(o2, 1, across[1], row[4], c2), put_slot(o2, 2, c3, 1, c2);
        put_slot(o3, 0, c1, 2, c3), put_slot(o3, 1, c2, 2, c3), put_slot(o3, 2, across[2], row[7], c3);
        return;
    }
    id -= a.nfa;
    if (id >= n_rows) return;
    // ---- the adjacency: a thread per row.  An old vertex keeps its row and gains V + s for every split face s it is a corner of,
    // ascending in s (columns stay ascending); a new vertex's row is its three corners, ascending, and itself
    const int r = (int)id;
    if (r == n_rows - 1) a.new_rowptr[n_rows] = a.nnz + 7 * a.s;
    if (r < a.nv) {
        const int o0 = a.rowptr[r], o1 = a.rowptr[r + 1];
        const int64_t i0 = a.inc_ptr[r], i1 = a.inc_ptr[r + 1];
        const int64_t start = o0 + i0;
        const float inv_len = 1.0f / (float)((o1 - o0) + (int)(i1 - i0));
        a.new_rowptr[r] = (int)start;
        if (o0 < 0 || o1 > a.nnz || i0 < 0 || i1 > 3 * (int64_t)a.s) return;
        for (int k = o0; k < o1; ++k) put_entry(a, start + (k - o0), r, a.col[k], inv_len);
        for (int64_t k = i0; k < i1; ++k) {
            const int64_t s = a.inc_item[k];
            if (s >= 0 && s < a.s) put_entry(a, start + (o1 - o0) + (k - i0), r, a.nv + s, inv_len);
        }
    } else {
        const int64_t s = r - a.nv, start = (int64_t)a.nnz + 3 * (int64_t)a.s + 4 * s;
        int64_t x = a.corners[3 * s], y = a.corners[3 * s + 1], z = a.corners[3 * s + 2], t;
        if (x > y) t = x, x = y, y = t;
        if (y > z) t = y, y = z, z = t;
        if (x > y) t = x, x = y, y = t;
        a.new_rowptr[r] = (int)start;
        if (x < 0 || z >= a.nv) return;
        put_entry(a, start, r, x, 0.25f), put_entry(a, start + 1, r, y, 0.25f), put_entry(a, start + 2, r, z, 0.25f);
        put_entry(a, start + 3, r, r, 0.25f);
    }
}

// ----------------------------------------------------------------------------------------------------- vertices ----
// THE launch rule of both directions: a work item is one (row, column group); a row has 3 position columns (always scalar: a
// [.,3] row is 12 bytes) and its feature columns in 16-byte groups of 4 when c % 4 == 0 and every feature pointer is 16-byte
// aligned, one by one otherwise.
struct SplitRoute {
    int width;         // feature columns per item: 4 or 1
    int per_row;       // items of a row: 3 + c / width
    int64_t items;
    unsigned blocks;
};

inline SplitRoute split_route(int64_t rows, int c, uintptr_t feature_ptr_bits)
{
    SplitRoute r;
    r.width = (c % 4 == 0 && (feature_ptr_bits & 15) == 0) ? 4 : 1;
    r.per_row = 3 + c / r.width;
    r.items = rows * r.per_row;
    r.blocks = (unsigned)((r.items + SPLIT_THREADS - 1) / SPLIT_THREADS);
    return r;
}

struct SplitVertexArgs {
    int nv, s, c;
    const float *verts, *feat;   // forward: inputs [nv,3] / [nv,c];  backward: the outputs' gradients [nv+s,3] / [nv+s,c]
    const int64_t *corners;      // forward [s,3]
    const int64_t *inc_ptr, *inc_item; // backward [nv+1] / [3s]
    float *out_v, *out_f;
    int per_row;
    int64_t items;
};

__device__ __forceinline__ float third_sum(float x, float y, float z) { return (x / 3.0f + y / 3.0f) + z / 3.0f; }

template <int WIDTH>
__global__ __launch_bounds__(SPLIT_THREADS) void split_vertices_fwd_kernel(SplitVertexArgs a)
{
    const int64_t id = (int64_t)blockIdx.x * SPLIT_THREADS + threadIdx.x;
    if (id >= a.items) return;
    const int64_t r = id / a.per_row;
    const int j = (int)(id - r * a.per_row);
    const bool is_new = r >= a.nv;
    int64_t x = 0, y = 0, z = 0;
    bool ok = true;
    if (is_new) {
        const int64_t s = r - a.nv;
        x = a.corners[3 * s], y = a.corners[3 * s + 1], z = a.corners[3 * s + 2];
        ok = x >= 0 && x < a.nv && y >= 0 && y < a.nv && z >= 0 && z < a.nv;
    }
    const float nan = __builtin_nanf("");
    if (j < 3) {
        float v = nan;
        if (!is_new) v = a.verts[3 * r + j];
        else if (ok) v = third_sum(a.verts[3 * x + j], a.verts[3 * y + j], a.verts[3 * z + j]);
        a.out_v[3 * r + j] = v;
        return;
    }
    const int64_t col = (int64_t)(j - 3) * WIDTH;
    if (WIDTH == 4) {
        float4 v = make_float4(nan, nan, nan, nan);
        if (!is_new) {
            v = *reinterpret_cast<const float4 *>(a.feat + r * a.c + col);
        } else if (ok) {
            const float4 fx = *reinterpret_cast<const float4 *>(a.feat + x * a.c + col);
            const float4 fy = *reinterpret_cast<const float4 *>(a.feat + y * a.c + col);
            const float4 fz = *reinterpret_cast<const float4 *>(a.feat + z * a.c + col);
            v = make_float4(third_sum(fx.x, fy.x, fz.x), third_sum(fx.y, fy.y, fz.y), third_sum(fx.z, fy.z, fz.z),
                            third_sum(fx.w, fy.w, fz.w));
        }
        *reinterpret_cast<float4 *>(a.out_f + r * a.c + col) = v;
    } else {
        float v = nan;
        if (!is_new) v = a.feat[r * a.c + col];
        else if (ok) v = third_sum(a.feat[x * a.c + col], a.feat[y * a.c + col], a.feat[z * a.c + col]);
        a.out_f[r * a.c + col] = v;
    }
}

// g_old[u] = g_out[u] + sum over the split faces s that have u as a corner, ascending in s, of g_out[V + s] / 3
template <int WIDTH>
__global__ __launch_bounds__(SPLIT_THREADS) void split_vertices_bwd_kernel(SplitVertexArgs a)
{
    const int64_t id = (int64_t)blockIdx.x * SPLIT_THREADS + threadIdx.x;
    if (id >= a.items) return;
    const int64_t u = id / a.per_row;
    const int j = (int)(id - u * a.per_row);
    int64_t k0 = a.inc_ptr[u], k1 = a.inc_ptr[u + 1];
    if (k0 < 0 || k1 > 3 * (int64_t)a.s) k0 = k1 = 0;
    if (j < 3) {
        float g = a.verts[3 * u + j];
        for (int64_t k = k0; k < k1; ++k) {
            const int64_t s = a.inc_item[k];
            if (s >= 0 && s < a.s) g += a.verts[3 * (a.nv + s) + j] / 3.0f;
        }
        a.out_v[3 * u + j] = g;
        return;
    }
    const int64_t col = (int64_t)(j - 3) * WIDTH;
    if (WIDTH == 4) {
        float4 g = *reinterpret_cast<const float4 *>(a.feat + u * a.c + col);
        for (int64_t k = k0; k < k1; ++k) {
            const int64_t s = a.inc_item[k];
            if (s < 0 || s >= a.s) continue;
            const float4 n = *reinterpret_cast<const float4 *>(a.feat + (a.nv + s) * a.c + col);
            g.x += n.x / 3.0f, g.y += n.y / 3.0f, g.z += n.z / 3.0f, g.w += n.w / 3.0f;
        }
        *reinterpret_cast<float4 *>(a.out_f + u * a.c + col) = g;
    } else {
        float g = a.feat[u * a.c + col];
        for (int64_t k = k0; k < k1; ++k) {
            const int64_t s = a.inc_item[k];
            if (s >= 0 && s < a.s) g += a.feat[(a.nv + s) * a.c + col] / 3.0f;
        }
        a.out_f[u * a.c + col] = g;
    }
}

// ============================================================================== a ragged batch: the union of B meshes ====
// The union is ONE mesh to the curvature, the tables and the vertices (an edge is still shared by exactly two faces); what a
// union needs of its own is a selection per mesh and index tables made by as many workgroups as it has chunks.  No workgroup
// waits on another inside a launch: every dependence between chunks is a launch boundary.
constexpr int SPLIT_CHUNK = SPLIT_THREADS; // items of a chunk of the running sums: one per thread

// sum of `mine` over the threads of the workgroup (a fixed tree over 256 values)
__device__ __forceinline__ int64_t block_sum(int64_t mine, int64_t *lds)
{
    __syncthreads(); // lds may still be read from a previous call
    lds[threadIdx.x] = mine;
    __syncthreads();
    for (int w = SPLIT_THREADS / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) lds[threadIdx.x] += lds[threadIdx.x + w];
        __syncthreads();
    }
    return lds[0];
}

// ------------------------------------------------------------------------------------------ selection per mesh ----
struct RaggedSelectArgs {
    int nfa, b;
    const float *curv;
    float angle;
    const int *row_list, *row_off; // the active rows grouped by mesh, ascending inside a mesh; where each group starts
    int64_t *stats;                // [b,4]: a mesh's count and the positions of its three largest curvatures
    int64_t *selected, *counts, *totals;
};

// the part [lo, hi) of mesh m's group that this thread walks: contiguous and in thread order, so the compaction is ordered
__device__ __forceinline__ void group_part(const RaggedSelectArgs &a, int m, int &lo, int &hi)
{
    int g0 = a.row_off[m], g1 = a.row_off[m + 1];
    g0 = g0 < 0 ? 0 : (g0 > a.nfa ? a.nfa : g0);
    g1 = g1 < g0 ? g0 : (g1 > a.nfa ? a.nfa : g1);
    const int64_t n = g1 - g0, per = (n + SPLIT_THREADS - 1) / SPLIT_THREADS, at = (int64_t)threadIdx.x * per;
    lo = g0 + (int)(at < n ? at : n);
    hi = (int64_t)lo + per < g1 ? lo + (int)per : g1;
}

__device__ __forceinline__ bool above(float c, float angle) { return (c * 180.0f) / 3.14159265358979323846f > angle; }

// what a mesh contributes to the list: its flagged rows, or below three of them as many of its three largest as exist
__device__ __forceinline__ int64_t mesh_entries(const int64_t *stats)
{
    if (stats[0] >= 3) return stats[0];
    return (stats[1] >= 0 ? 1 : 0) + (stats[2] >= 0 ? 1 : 0) + (stats[3] >= 0 ? 1 : 0);
}

// The list top3_insert keeps, in named registers (an array indexed by a loop variable lives in scratch memory): the same rule.
struct Top3 {
    float v0 = 0.f, v1 = 0.f, v2 = 0.f;
    int i0 = -1, i1 = -1, i2 = -1;
    __device__ __forceinline__ void insert(float v, int i)
    {
        if (v != v || i < 0) return; // a degenerate face is never selected
        if (ahead(v, i, v0, i0)) v2 = v1, i2 = i1, v1 = v0, i1 = i0, v0 = v, i0 = i;
        else if (ahead(v, i, v1, i1)) v2 = v1, i2 = i1, v1 = v, i1 = i;
        else if (ahead(v, i, v2, i2)) v2 = v, i2 = i;
    }
};

// Launch 1, a workgroup per mesh: stats[m] = {count, top3} of face_select_kernel taken over the mesh's rows alone.
__global__ __launch_bounds__(SPLIT_THREADS) void face_select_ragged_stats_kernel(RaggedSelectArgs a)
{
    __shared__ int64_t lds64[SPLIT_THREADS];
    __shared__ float cand_v[3 * SPLIT_THREADS];
    __shared__ int cand_i[3 * SPLIT_THREADS];
    const int t = threadIdx.x, m = blockIdx.x;
    int lo, hi;
    group_part(a, m, lo, hi);
    Top3 mine;
    int n = 0;
    for (int g = lo; g < hi; ++g) {
        const int i = a.row_list[g];
        if (i < 0 || i >= a.nfa) continue;
        const float c = a.curv[i];
        n += above(c, a.angle) ? 1 : 0;
        mine.insert(c, i);
    }
    const int64_t run = block_sum(n, lds64);
    // the lists merge pairwise: ahead() is a strict order on (curvature, position) pairs, so the three of a union that are
    // ahead of all others do not depend on the order of the merges
    const auto keep = [&] {
        cand_v[3 * t] = mine.v0, cand_v[3 * t + 1] = mine.v1, cand_v[3 * t + 2] = mine.v2;
        cand_i[3 * t] = mine.i0, cand_i[3 * t + 1] = mine.i1, cand_i[3 * t + 2] = mine.i2;
    };
    keep();
    __syncthreads();
    for (int w = SPLIT_THREADS / 2; w > 0; w >>= 1) {
        if (t < w) { // reads the list of thread t + w, which no thread writes in this step
            for (int k = 0; k < 3; ++k) mine.insert(cand_v[3 * (t + w) + k], cand_i[3 * (t + w) + k]);
            keep();
        }
        __syncthreads();
    }
    if (t != 0) return;
    int64_t *out = a.stats + 4 * (int64_t)m;
    out[0] = run, out[1] = mine.i0, out[2] = mine.i1, out[3] = mine.i2;
}

// Launch 2, a workgroup per mesh: it adds up what the meshes in front of it contribute and writes its own entries there.
// counts[m] = its entries; the last workgroup writes totals = {S, the meshes with fewer than three faces that have a curvature}.
__global__ __launch_bounds__(SPLIT_THREADS) void face_select_ragged_write_kernel(RaggedSelectArgs a)
{
    __shared__ int lds[SPLIT_THREADS];
    __shared__ int64_t lds64[SPLIT_THREADS];
    const int t = threadIdx.x, m = blockIdx.x;
    const int64_t cap = (int64_t)a.nfa + 3 * (int64_t)a.b;
    int64_t part = 0;
    for (int q = t; q < m; q += SPLIT_THREADS) part += mesh_entries(a.stats + 4 * (int64_t)q);
    const int64_t base = block_sum(part, lds64);
    const int64_t *own = a.stats + 4 * (int64_t)m;
    const int64_t mine = mesh_entries(own);
    if (own[0] >= 3) {
        int lo, hi;
        group_part(a, m, lo, hi);
        int n = 0;
        for (int g = lo; g < hi; ++g) {
            const int i = a.row_list[g];
            if (i >= 0 && i < a.nfa) n += above(a.curv[i], a.angle) ? 1 : 0;
        }
        int64_t at = base + block_offset(n, lds);
        for (int g = lo; g < hi; ++g) {
            const int i = a.row_list[g];
            if (i < 0 || i >= a.nfa || !above(a.curv[i], a.angle)) continue;
            if (at >= 0 && at < cap) a.selected[at] = i;
            ++at;
        }
    } else if (t == 0) {
        int64_t at = base;
        for (int k = 1; k <= 3; ++k)
            if (own[k] >= 0 && at < cap) a.selected[at++] = own[k];
    }
    if (t == 0) a.counts[m] = mine;
    if (m != a.b - 1) return;
    int64_t bad = 0;
    for (int q = t; q < a.b; q += SPLIT_THREADS) {
        const int64_t *s = a.stats + 4 * (int64_t)q;
        bad += (s[0] < 3 && s[3] < 0) ? 1 : 0;
    }
    bad = block_sum(bad, lds64);
    if (t == 0) a.totals[0] = base + mine, a.totals[1] = bad;
}

// ------------------------------------------------------------------------------- index tables over many chunks ----
struct RaggedIndexArgs {
    int nv, nft, nfa, s;
    const int64_t *faces, *face_list, *splitting, *vert_mesh, *face_mesh;
    int64_t *corners, *split_pos, *unsplit_rank, *face_s, *inc_ptr, *inc_item, *vert_mesh_new, *face_mesh_new;
    // the workspace (ragged_index_layout): zero at the first launch up to `slot`
    int64_t *count;   // [nv]   how many split faces have the vertex as a corner
    int64_t *vtot;    // [chunks of nv]   the same per chunk of vertices
    int64_t *rtot;    // [chunks of nfa]  split rows per chunk of rows
    int64_t *sp_tmp;  // [nfa]  k + 1 at splitting[k]
    int64_t *fs_tmp;  // [nft]  k + 1 at the face of splitting[k]
    int64_t *slot;    // [3s]   the order in which corner j of split face k arrived at its vertex
};

inline int64_t chunks_of(int64_t n) { return (n + SPLIT_CHUNK - 1) / SPLIT_CHUNK; }
inline int64_t ragged_index_zeroed_words(int nv, int nft, int nfa) { return nv + chunks_of(nv) + chunks_of(nfa) + (int64_t)nfa + nft; }

__device__ __forceinline__ int64_t count_up(int64_t *p) { return (int64_t)atomicAdd(reinterpret_cast<unsigned long long *>(p), 1ull); }

// Launch 1, a thread per split face: the scatter, the corners, the new ids, and integer counts -- per vertex (the value the
// atomic returns is kept: it is the corner's place in the vertex's row until the sort), per chunk of vertices, per chunk of rows.
__global__ __launch_bounds__(SPLIT_THREADS) void face_split_scatter_ragged_kernel(RaggedIndexArgs a)
{
    const int64_t k = (int64_t)blockIdx.x * SPLIT_THREADS + threadIdx.x;
    if (k >= a.s) return;
    const int64_t p = a.splitting[k];
    int64_t c[3] = {-1, -1, -1}, mesh = -1;
    if (p >= 0 && p < a.nfa) {
        a.sp_tmp[p] = k + 1;
        count_up(a.rtot + p / SPLIT_CHUNK);
        const int64_t own = a.face_list[9 * p + 2];
        if (own >= 0 && own < a.nft) {
            a.fs_tmp[own] = k + 1;
            for (int j = 0; j < 3; ++j) c[j] = a.faces[3 * own + j];
            mesh = a.face_mesh[own];
        }
    }
    for (int j = 0; j < 3; ++j) {
        int64_t place = -1;
        if (c[j] >= 0 && c[j] < a.nv) {
            place = count_up(a.count + c[j]);
            count_up(a.vtot + c[j] / SPLIT_CHUNK);
        }
        a.corners[3 * k + j] = c[j];
        a.slot[3 * k + j] = place;
        a.face_mesh_new[(int64_t)a.nft + j * (int64_t)a.s + k] = mesh;
    }
    a.vert_mesh_new[(int64_t)a.nv + k] = mesh;
}

// Launch 2, a workgroup per chunk: the two running sums (the chunk's own, on top of the totals of the chunks in front of it),
// the tables in their final form, the old ids copied.
__global__ __launch_bounds__(SPLIT_THREADS) void face_split_scan_ragged_kernel(RaggedIndexArgs a)
{
    __shared__ int lds[SPLIT_THREADS];
    __shared__ int64_t lds64[SPLIT_THREADS];
    const int t = threadIdx.x;
    const int64_t chunk = blockIdx.x, i = chunk * SPLIT_CHUNK + t;
    if (chunk * SPLIT_CHUNK < a.nfa) { // unsplit_rank[i] = how many unsplit rows precede row i
        int64_t part = 0;
        for (int64_t q = t; q < chunk; q += SPLIT_THREADS) part += a.rtot[q];
        const int64_t split_before = block_sum(part, lds64);
        const int64_t k = i < a.nfa ? a.sp_tmp[i] - 1 : 0;
        const int within = block_offset((i < a.nfa && k < 0) ? 1 : 0, lds);
        if (i < a.nfa) a.split_pos[i] = k, a.unsplit_rank[i] = chunk * SPLIT_CHUNK - split_before + within;
    }
    if (chunk * SPLIT_CHUNK < a.nv) { // inc_ptr[u + 1] = the counts up to and with vertex u
        int64_t part = 0;
        for (int64_t q = t; q < chunk; q += SPLIT_THREADS) part += a.vtot[q];
        const int64_t before = block_sum(part, lds64);
        const int n = i < a.nv ? (int)a.count[i] : 0;
        const int within = block_offset(n, lds);
        if (i < a.nv) a.inc_ptr[i + 1] = before + within + n, a.vert_mesh_new[i] = a.vert_mesh[i];
    }
    if (i == 0) a.inc_ptr[0] = 0;
    if (i < a.nft) a.face_s[i] = a.fs_tmp[i] - 1, a.face_mesh_new[i] = a.face_mesh[i];
    if (i < 3 * (int64_t)a.s) a.inc_item[i] = -1;
}

// Launch 3, a thread per corner of a split face: the incidence rows, each corner at the place it arrived at.
__global__ __launch_bounds__(SPLIT_THREADS) void face_split_fill_ragged_kernel(RaggedIndexArgs a)
{
    const int64_t e = (int64_t)blockIdx.x * SPLIT_THREADS + threadIdx.x;
    if (e >= 3 * (int64_t)a.s) return;
    const int64_t c = a.corners[e], place = a.slot[e];
    if (c < 0 || c >= a.nv || place < 0) return;
    const int64_t at = a.inc_ptr[c] + place;
    if (at >= 0 && at < a.inc_ptr[c + 1] && at < 3 * (int64_t)a.s) a.inc_item[at] = e / 3;
}

// Launch 4, a thread per vertex: ascending split order within its row, which hides the order the atomics were served in.
__global__ __launch_bounds__(SPLIT_THREADS) void face_split_sort_ragged_kernel(RaggedIndexArgs a)
{
    const int64_t u = (int64_t)blockIdx.x * SPLIT_THREADS + threadIdx.x;
    if (u >= a.nv) return;
    const int64_t lo = a.inc_ptr[u], hi = a.inc_ptr[u + 1];
    if (lo < 0 || hi > 3 * (int64_t)a.s) return;
    for (int64_t i = lo + 1; i < hi; ++i) {
        const int64_t v = a.inc_item[i];
        int64_t j = i;
        for (; j > lo && a.inc_item[j - 1] > v; --j) a.inc_item[j] = a.inc_item[j - 1];
        a.inc_item[j] = v;
    }
}

} // namespace

extern "C" int geom_face_select_ragged_f32(int nfa, const float *curvature, float angle, int b, const int *row_list,
                                           const int *row_off, int64_t *stats, int64_t *selected, int64_t *counts,
                                           int64_t *totals, void *stream)
{
    if (nfa < 0 || b < 0) return GEOM_EINVAL;
    if (!totals || (nfa > 0 && (!curvature || !row_list))) return GEOM_EINVAL;
    if (b > 0 && (!row_off || !stats || !selected || !counts)) return GEOM_EINVAL;
    hipStream_t q = static_cast<hipStream_t>(stream);
    if (b == 0) return hipMemsetAsync(totals, 0, 2 * sizeof(int64_t), q) == hipSuccess ? 0 : geom::launch_status();
    RaggedSelectArgs a{nfa, b, curvature, angle, row_list, row_off, stats, selected, counts, totals};
    hipLaunchKernelGGL(face_select_ragged_stats_kernel, dim3(b), dim3(SPLIT_THREADS), 0, q, a);
    hipLaunchKernelGGL(face_select_ragged_write_kernel, dim3(b), dim3(SPLIT_THREADS), 0, q, a);
    return geom::launch_status();
}

extern "C" int64_t geom_face_split_index_ragged_words(int nv, int nft, int nfa, int s)
{
    if (nv < 0 || nft < 0 || nfa < 0 || s < 0) return GEOM_EINVAL;
    return ragged_index_zeroed_words(nv, nft, nfa) + 3 * (int64_t)s;
}

extern "C" int geom_face_split_index_ragged(int nv, int nft, const int64_t *faces, int nfa, const int64_t *face_list, int s,
                                            const int64_t *splitting, const int64_t *vert_mesh, const int64_t *face_mesh,
                                            int64_t *corners, int64_t *split_pos, int64_t *unsplit_rank, int64_t *face_s,
                                            int64_t *inc_ptr, int64_t *inc_item, int64_t *vert_mesh_new, int64_t *face_mesh_new,
                                            int64_t *workspace, void *stream)
{
    if (nv < 0 || nft < 0 || nfa < 0 || s < 0 || s > nfa) return GEOM_EINVAL;
    if (!inc_ptr || !workspace) return GEOM_EINVAL;
    if (nft > 0 && (!faces || !face_s || !face_mesh)) return GEOM_EINVAL;
    if (nfa > 0 && (!face_list || !split_pos || !unsplit_rank)) return GEOM_EINVAL;
    if (nv > 0 && !vert_mesh) return GEOM_EINVAL;
    if (nv + s > 0 && !vert_mesh_new) return GEOM_EINVAL;
    if (nft + s > 0 && !face_mesh_new) return GEOM_EINVAL;
    if (s > 0 && (!splitting || !corners || !inc_item)) return GEOM_EINVAL;
    if (3 * (int64_t)s > INT_MAX || (int64_t)nft + 3 * (int64_t)s > INT_MAX || (int64_t)nv + s > INT_MAX) return GEOM_ETOOBIG;
    hipStream_t q = static_cast<hipStream_t>(stream);
    const int64_t zeroed = ragged_index_zeroed_words(nv, nft, nfa);
    RaggedIndexArgs a{nv, nft, nfa, s, faces, face_list, splitting, vert_mesh, face_mesh, corners, split_pos, unsplit_rank, face_s,
                      inc_ptr, inc_item, vert_mesh_new, face_mesh_new};
    a.count = workspace;
    a.vtot = a.count + nv;
    a.rtot = a.vtot + chunks_of(nv);
    a.sp_tmp = a.rtot + chunks_of(nfa);
    a.fs_tmp = a.sp_tmp + nfa;
    a.slot = workspace + zeroed;
    if (zeroed > 0 && hipMemsetAsync(workspace, 0, zeroed * sizeof(int64_t), q) != hipSuccess) return geom::launch_status();
    const auto blocks = [](int64_t items) { return dim3((unsigned)((items + SPLIT_THREADS - 1) / SPLIT_THREADS)); };
    int64_t widest = nfa > nv ? nfa : nv;
    widest = nft > widest ? nft : widest;
    widest = 3 * (int64_t)s > widest ? 3 * (int64_t)s : widest;
    if (s > 0) hipLaunchKernelGGL(face_split_scatter_ragged_kernel, blocks(s), dim3(SPLIT_THREADS), 0, q, a);
    hipLaunchKernelGGL(face_split_scan_ragged_kernel, blocks(widest > 0 ? widest : 1), dim3(SPLIT_THREADS), 0, q, a);
    if (s > 0) hipLaunchKernelGGL(face_split_fill_ragged_kernel, blocks(3 * (int64_t)s), dim3(SPLIT_THREADS), 0, q, a);
    if (s > 0 && nv > 0) hipLaunchKernelGGL(face_split_sort_ragged_kernel, blocks(nv), dim3(SPLIT_THREADS), 0, q, a);
    return geom::launch_status();
}

extern "C" int geom_face_curvature_f32(int nv, const float *verts, int nft, const int64_t *faces, int nfa,
                                       const int64_t *face_list, float *curvature, void *stream)
{
    if (nv < 0 || nft < 0 || nfa < 0) return GEOM_EINVAL;
    if (nfa == 0) return 0;
    if (!verts || !faces || !face_list || !curvature) return GEOM_EINVAL;
    hipLaunchKernelGGL(face_curvature_kernel, dim3((nfa + SPLIT_THREADS - 1) / SPLIT_THREADS), dim3(SPLIT_THREADS), 0,
                       static_cast<hipStream_t>(stream), nv, verts, nft, faces, nfa, face_list, curvature);
    return geom::launch_status();
}

extern "C" int geom_face_select_f32(int nfa, const float *curvature, float angle, int64_t *selected, int64_t *count_top3,
                                    void *stream)
{
    if (nfa < 0) return GEOM_EINVAL;
    if (!count_top3 || (nfa > 0 && (!curvature || !selected))) return GEOM_EINVAL;
    hipLaunchKernelGGL(face_select_kernel, dim3(1), dim3(SPLIT_THREADS), 0, static_cast<hipStream_t>(stream), nfa, curvature,
                       angle, selected, count_top3);
    return geom::launch_status();
}

extern "C" int geom_face_split_index(int nv, int nft, const int64_t *faces, int nfa, const int64_t *face_list, int s,
                                     const int64_t *splitting, int64_t *corners, int64_t *split_pos, int64_t *unsplit_rank,
                                     int64_t *face_s, int64_t *inc_ptr, int64_t *inc_item, int64_t *cursor, void *stream)
{
    if (nv < 0 || nft < 0 || nfa < 0 || s < 0 || s > nfa) return GEOM_EINVAL;
    if (!inc_ptr) return GEOM_EINVAL;
    if (nft > 0 && (!faces || !face_s)) return GEOM_EINVAL;
    if (nfa > 0 && (!face_list || !split_pos || !unsplit_rank)) return GEOM_EINVAL;
    if (nv > 0 && !cursor) return GEOM_EINVAL;
    if (s > 0 && (!splitting || !corners || !inc_item)) return GEOM_EINVAL;
    SplitIndexArgs a{nv, nft, nfa, s, faces, face_list, splitting, corners, split_pos, unsplit_rank, face_s, inc_ptr, inc_item, cursor};
    hipLaunchKernelGGL(face_split_index_kernel, dim3(1), dim3(SPLIT_THREADS), 0, static_cast<hipStream_t>(stream), a);
    return geom::launch_status();
}

extern "C" int geom_face_split_tables(const geom_face_split *args, void *stream)
{
    if (!args) return GEOM_EINVAL;
    const geom_face_split &a = *args;
    if (a.nv < 0 || a.nft < 0 || a.nfa < 0 || a.s < 0 || a.nnz < 0 || a.s > a.nfa) return GEOM_EINVAL;
    if ((int64_t)a.nnz + 7 * (int64_t)a.s > INT_MAX || (int64_t)a.nft + 3 * (int64_t)a.s > INT_MAX) return GEOM_ETOOBIG;
    if (!a.new_rowptr) return GEOM_EINVAL;
    if (a.nft > 0 && (!a.faces || !a.face_s)) return GEOM_EINVAL;
    if (a.nft + a.s > 0 && !a.new_faces) return GEOM_EINVAL;
    if (a.nfa > 0 && (!a.face_list || !a.split_pos || !a.unsplit_rank || !a.new_face_list)) return GEOM_EINVAL;
    if (a.nv > 0 && (!a.rowptr || !a.inc_ptr)) return GEOM_EINVAL;
    if (a.nnz > 0 && !a.col) return GEOM_EINVAL;
    if (a.s > 0 && (!a.corners || !a.inc_item)) return GEOM_EINVAL;
    if (a.nnz + a.s > 0 && (!a.new_col || !a.new_val || !a.new_val_t || !a.new_ones)) return GEOM_EINVAL;
    const int64_t items = ((int64_t)a.nft + 3 * (int64_t)a.s) + a.nfa + ((int64_t)a.nv + a.s);
    if (items == 0) { // an empty mesh: the one element of the new rowptr is its end
        return hipMemsetAsync(a.new_rowptr, 0, sizeof(int), static_cast<hipStream_t>(stream)) == hipSuccess ? 0 : geom::launch_status();
    }
    hipLaunchKernelGGL(face_split_tables_kernel, dim3((unsigned)((items + SPLIT_THREADS - 1) / SPLIT_THREADS)), dim3(SPLIT_THREADS),
                       0, static_cast<hipStream_t>(stream), a);
    return geom::launch_status();
}

extern "C" int geom_split_vertices_fwd_f32(int nv, int s, int c, const float *verts, const float *features,
                                           const int64_t *corners, float *out_verts, float *out_features, void *stream)
{
    if (nv < 0 || s < 0 || c < 0) return GEOM_EINVAL;
    const int64_t rows = (int64_t)nv + s;
    if (rows == 0) return 0;
    if (!verts || !out_verts || (c > 0 && (!features || !out_features)) || (s > 0 && !corners)) return GEOM_EINVAL;
    if (s > 0 && nv == 0) return GEOM_EINVAL;
    const SplitRoute r = split_route(rows, c, (uintptr_t)features | (uintptr_t)out_features);
    SplitVertexArgs a{nv, s, c, verts, features, corners, nullptr, nullptr, out_verts, out_features, r.per_row, r.items};
    if (r.width == 4)
        hipLaunchKernelGGL(split_vertices_fwd_kernel<4>, dim3(r.blocks), dim3(SPLIT_THREADS), 0, static_cast<hipStream_t>(stream), a);
    else
        hipLaunchKernelGGL(split_vertices_fwd_kernel<1>, dim3(r.blocks), dim3(SPLIT_THREADS), 0, static_cast<hipStream_t>(stream), a);
    return geom::launch_status();
}

extern "C" int geom_split_vertices_bwd_f32(int nv, int s, int c, const float *grad_out_verts, const float *grad_out_features,
                                           const int64_t *inc_ptr, const int64_t *inc_item, float *grad_verts,
                                           float *grad_features, void *stream)
{
    if (nv < 0 || s < 0 || c < 0) return GEOM_EINVAL;
    if (nv == 0) return 0;
    if (!grad_out_verts || !grad_verts || (c > 0 && (!grad_out_features || !grad_features)) || !inc_ptr || (s > 0 && !inc_item))
        return GEOM_EINVAL;
    const SplitRoute r = split_route(nv, c, (uintptr_t)grad_out_features | (uintptr_t)grad_features);
    SplitVertexArgs a{nv, s, c, grad_out_verts, grad_out_features, nullptr, inc_ptr, inc_item, grad_verts, grad_features,
                      r.per_row, r.items};
    if (r.width == 4)
        hipLaunchKernelGGL(split_vertices_bwd_kernel<4>, dim3(r.blocks), dim3(SPLIT_THREADS), 0, static_cast<hipStream_t>(stream), a);
    else
        hipLaunchKernelGGL(split_vertices_bwd_kernel<1>, dim3(r.blocks), dim3(SPLIT_THREADS), 0, static_cast<hipStream_t>(stream), a);
    return geom::launch_status();
}
