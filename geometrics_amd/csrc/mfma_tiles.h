// The two exact-fp32 tile products on the gfx950 matrix cores (v_mfma_f32_16x16x4_f32) that more than one kernel file runs:
// the layouts, the k permutations and the lane maps, stated once.  How a panel is FILLED and how a result leaves for memory
// stay with the kernels: those are their schedules.
#pragma once
#include "buffer_access.h"

namespace geom {

// probe builds (tools/probe/*_variants.sh) compile a phase out of a product; 0 in the library
enum { TILE_PROBE_NONE = 0, TILE_PROBE_NO_FRAG, TILE_PROBE_NO_MFMA, TILE_PROBE_FEW_MFMA };

// ---- the weight-stationary 16 x 192 row-block product (zn_stack.hip, deform_block.hip) ----------------------------------
// C[16][192] = X[16][192] . W[192][192].  The weight never touches LDS: wave w of four owns output columns 48 w .. 48 w + 47
// and keeps its 192 x 48 slice in 144 registers -- lane (x, g), MFMA step (jp, c), u = 0..2: W[k = 48 g + 4 jp + c][48 w +
// 3 x + u].  The activation row-block lies in LDS as a panel [k-quarter g][row][52]: the four lane groups of a ds_read_b128
// never share a bank (row pitch 13 x 16 B, odd; quarter pitch 832 floats, a multiple of 64 dwords), and ONE 16-byte fragment
// read of lane (x, g) -- row x, k = 48 g + 4 jp .. + 3 -- feeds four k-steps = 12 MFMAs.  The result leaves through a staging
// tile [row][196] (196 % 32 == 4: the b128 writes of 8 rows hit 32 banks) so that it is stored in memory order.
constexpr int RB_C = 192;           // inner dimension = output columns
constexpr int RB_LDR = 52;          // floats per (quarter, row) line of the panel: 48 used
constexpr int RB_SUB = 16 * RB_LDR; // one k-quarter of the panel
constexpr int RB_PANEL = 4 * RB_SUB;
constexpr int RB_LDC = RB_C + 4;    // row pitch of the staging tile
constexpr int RB_CST = 16 * RB_LDC; // one 16 x 192 staging tile

// float offset of element (row, col) inside a panel: quarter col / 48, position col % 48
__device__ __forceinline__ int panel_offset(int col, int row) { return (col / 48) * RB_SUB + row * RB_LDR + col % 48; }

// acc = panel . slice for lane (x, g): `pa` = the lane's line of the panel (panel + panel_offset(48 g, x)), weight(jp, c, u) the
// slice element above.  The next group's fragment is requested in front of this group's 12 MFMAs (fenced: the compiler
// otherwise sinks the read to its use and every group starts with an LDS round trip).  The weight is the instruction's first
// operand: accumulator u holds C[row x][48 wave + 12 g + 3 r + u], r = 0..3.
template <int PROBE = TILE_PROBE_NONE, typename Weight>
__device__ __forceinline__ void rowblock_product(Weight weight, const float *pa, f32x4 (&acc)[3])
{
#pragma unroll
    for (int u = 0; u < 3; ++u) acc[u] = (f32x4){0.f, 0.f, 0.f, 0.f};
    f32x4 af = *reinterpret_cast<const f32x4 *>(pa);
#pragma unroll
    for (int jp = 0; jp < 12; ++jp) {
        f32x4 an = af;
        if (jp + 1 < 12) an = *reinterpret_cast<const f32x4 *>(pa + 4 * (jp + 1));
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            if (PROBE == TILE_PROBE_FEW_MFMA && jp >= 2) continue; // a sixth of the MFMAs (wrong results)
#pragma unroll
            for (int u = 0; u < 3; ++u) {
                if (PROBE == TILE_PROBE_NO_MFMA) acc[u] = acc[u] + af * weight(jp, c, u);
                else acc[u] = __builtin_amdgcn_mfma_f32_16x16x4f32(weight(jp, c, u), af[c], acc[u], 0, 0, 0);
            }
        }
        __builtin_amdgcn_sched_barrier(0);
        af = an;
    }
}

// the lane's twelve consecutive columns into the staging tile (natural [row][col] layout, pitch RB_LDC)
__device__ __forceinline__ void rowblock_to_stage(const f32x4 (&acc)[3], float *stage, int wave, int x, int g)
{
    float e[12];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int u = 0; u < 3; ++u) e[3 * r + u] = acc[u][r];
    float *dst = stage + x * RB_LDC + wave * 48 + 12 * g;
#pragma unroll
    for (int v = 0; v < 3; ++v) *reinterpret_cast<f32x4 *>(dst + 4 * v) = (f32x4){e[4 * v], e[4 * v + 1], e[4 * v + 2], e[4 * v + 3]};
}

// ---- the staged 64 x 64 tile (dense_any.hip, encoder_stack.hip) ----------------------------------------------------------
// C tile = A panel . B panel over a BK-deep stage, both panels in LDS, four waves 2 x 2, a wave 16 WM x 32 = WM x 2 MFMA tiles.
// A panel of an operand whose SUMMED index is contiguous in memory ("k-contiguous") is kept as [row][BK + 4] and a lane reads
// FOUR consecutive k of its row with one ds_read_b128; a panel whose summed index is the slow one ("k-major") is kept as
// [k][rows + 4] and read one float per MFMA.  The k-steps of a stage are permuted so that both forms agree: step s of quarter
// qq gives lane group g the summed index 16 qq + 4 g + s.  Bank arithmetic: [row][36] -- the 8 lanes a b128 read serves per
// cycle sit 36 floats apart = 4 banks: 32 distinct banks; [k][68] -- lane groups g, g + 1 sit 4 * 68 floats = 16 banks apart,
// 16 lanes each: 32 distinct banks.  The accumulators are taken with the operands swapped (D^T = B^T A^T) so that a lane holds
// four consecutive COLUMNS of one row.
constexpr int TILE_N = 64;                           // columns of the tile
constexpr int tile_pk(int bk) { return bk + 4; }     // [row][k] panel pitch (36 / 20 floats: 8 lanes x 4 banks apart)
constexpr int tile_pm(int rows) { return rows + 4; } // [k][row] panel pitch (68 / 132: 4 mod 8)
constexpr int tile_panel(int rows, int bk) { return rows * tile_pk(bk) > bk * tile_pm(rows) ? rows * tile_pk(bk) : bk * tile_pm(rows); } // floats per buffer

// the wave's first row / column inside the tile
template <int WM>
__device__ __forceinline__ int tile_wave_row(int wave) { return 16 * WM * (wave >> 1); }
__device__ __forceinline__ int tile_wave_col(int wave) { return 32 * (wave & 1); }

// one stage: A_KM / B_KN = the panel is k-major ([k][32 WM + 4] / [k][68]), else [row][BK + 4]
template <bool A_KM, bool B_KN, int WM, int BK, int PROBE = TILE_PROBE_NONE>
__device__ __forceinline__ void tile_stage(const float *as, const float *bs, int wr, int wc, int x, int g, f32x4 (&acc)[WM][2])
{
    constexpr int PK = tile_pk(BK), PMA = tile_pm(32 * WM), PMB = tile_pm(TILE_N);
#pragma unroll
    for (int qq = 0; qq < BK / 16; ++qq) {
        f32x4 a4[WM], b4[2];
        if (PROBE == TILE_PROBE_NO_FRAG && qq > 0) { // the fragments of the first quarter-stage feed every MFMA (no further LDS reads)
#pragma unroll
            for (int s = 0; s < 4; ++s)
#pragma unroll
                for (int i = 0; i < WM; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(acc[i][j ^ 1][0], acc[i ^ 1][j][1], acc[i][j], 0, 0, 0);
            continue;
        }
        if constexpr (!A_KM) {
#pragma unroll
            for (int i = 0; i < WM; ++i) a4[i] = *reinterpret_cast<const f32x4 *>(as + (wr + 16 * i + x) * PK + 16 * qq + 4 * g);
        }
        if constexpr (!B_KN) {
#pragma unroll
            for (int j = 0; j < 2; ++j) b4[j] = *reinterpret_cast<const f32x4 *>(bs + (wc + 16 * j + x) * PK + 16 * qq + 4 * g);
        }
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            float af[WM], bf[2];
            const int kk = 16 * qq + 4 * g + s;
#pragma unroll
            for (int i = 0; i < WM; ++i) af[i] = A_KM ? as[kk * PMA + wr + 16 * i + x] : a4[i][s];
#pragma unroll
            for (int j = 0; j < 2; ++j) bf[j] = B_KN ? bs[kk * PMB + wc + 16 * j + x] : b4[j][s];
#pragma unroll
            for (int i = 0; i < WM; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(bf[j], af[i], acc[i][j], 0, 0, 0);
        }
    }
}

// the epilogue's walk: lane (x, g) holds C[m][n .. n + 3] = acc[i][j] with m = mw + 16 i + x, n = nw + 16 j + 4 g, where
// (mw, nw) is the wave's first row / column in the matrix; out(m, n, acc[i][j]) per accumulator
template <int WM, typename Out>
__device__ __forceinline__ void tile_for_each_output(const f32x4 (&acc)[WM][2], int mw, int nw, int x, int g, Out out)
{
#pragma unroll
    for (int i = 0; i < WM; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) out(mw + 16 * i + x, nw + 16 * j + 4 * g, acc[i][j]);
}

} // namespace geom
