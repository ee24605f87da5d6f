"""The face sampler's arithmetic on the host (tests/draw_helpers.py restates csrc/draw_body.h operation for operation; tests/
test_draw_exact_gpu.py holds the kernels to that restatement bit for bit): the Philox stream against the Random123 known answers,
and the draw, for EVERY ONE of the 2^24 uniforms a sample can get, against the float64 inverse CDF of the same fp32 vertices."""
import functools

import numpy as np
import pytest

import draw_helpers as dh

KNOWN_ANSWERS = [      # Random123 kat_vectors, philox4x32-10: counter, key, output
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


def test_philox_known_answers():
    for ctr, key, out in KNOWN_ANSWERS:
        assert [hex(int(w)) for w in dh.philox4x32_10(ctr, key)] == [hex(w) for w in out]
    # vectorised over the leading axes, one key for all or one each
    ctrs = np.array([k[0] for k in KNOWN_ANSWERS], dtype=np.uint64)
    keys = np.array([k[1] for k in KNOWN_ANSWERS], dtype=np.uint64)
    assert np.array_equal(dh.philox4x32_10(ctrs, keys), np.array([k[2] for k in KNOWN_ANSWERS], dtype=np.uint32))
    assert np.array_equal(dh.philox4x32_10(ctrs[2:], KNOWN_ANSWERS[2][1])[0], np.array(KNOWN_ANSWERS[2][2], dtype=np.uint32))


def test_stream_layout_and_u01():
    """counter = (sample, global mesh truncated to 32 bits, position low, position high), key = (seed low, seed high); u01 keeps
    the 24 high bits."""
    seed, pos, mesh = 0x123456789ABCDEF0 & (2 ** 63 - 1), (7 << 32) | 5, (5 << 24) + 2
    w = dh.stream_words(seed, pos, mesh, 4)
    assert np.array_equal(w[3], dh.philox4x32_10((3, mesh, 5, 7), (0x9ABCDEF0, 0x12345678)))
    assert np.array_equal(dh.stream_words(seed, pos, mesh + (1 << 32), 4), w)          # truncated
    assert not np.array_equal(dh.stream_words(seed, pos + (1 << 32), mesh, 4), w)      # the position's high half counts
    x = np.array([0, 0xff, 0x100, 0xffffffff, 0x80000000], dtype=np.uint32)
    u = dh.u01(x)
    assert u.dtype == np.float32 and np.array_equal(u.astype(np.float64), [0, 0, 2.0 ** -24, 1 - 2.0 ** -24, 0.5])
    r0, r1, r2 = dh.stream_uniforms(seed, pos, mesh, 4)
    assert np.array_equal(r0, dh.u01(w[:, 0])) and np.array_equal(r1, dh.u01(w[:, 1])) and np.array_equal(r2, dh.u01(w[:, 2]))


CASES = [(nf, "plain") for nf in (1, 2, 20, 1023, 1024, 1025, 16384)] + \
        [(nf, "ends") for nf in (20, 1025, 16384)] + [(nf, "dominant") for nf in (20, 1025)]


@functools.lru_cache(maxsize=None)
def _soup(nf, variant):
    return dh.triangle_soup(nf, 1000 + nf, variant)


@pytest.mark.parametrize("nf,variant", CASES, ids=["%d-%s" % c for c in CASES])
def test_every_uniform_against_the_float64_inverse_cdf(nf, variant):
    """All 2^24 uniforms through the restated draw, on triangle soups with one face in ten of exactly zero area (and with the first
    and last face degenerate; and with one face of > 99 % of the area), at face counts that leave threads without faces (1, 2,
    20), fill all but one / exactly all 1024 threads with one face, give 513 threads two faces (1025: the other 511 own none), and
    fill the table (16384):

      * the table never steps down and is flat across every zero-area face, so no such face is ever drawn;
      * the face drawn never decreases with the uniform, and every face the float64 inverse CDF draws is drawn;
      * every face's count lies within K = draw_helpers.count_bound of its float64 count: 2 * (per + 6 + 15 + 8), one grid point
        per fp32 rounding on the way to a table entry, two boundaries a face (derived there): 60 up to 1024 faces, 62 at 1025,
        90 at 16384.  Measured worst difference over all twelve cases: 3.

    The table is the running maximum, over the faces that weigh something, of the fp32 scanned sums.  The sums alone (the table
    up to this test) fail the first two lines on these soups: 1 / 17 / 9 / 17 descending steps, 2 / 30 / 17 / 30 zero-area faces
    with a step of their own and 1 / 12 / 8 / 11 uniforms that draw one, at 20 / 1023 / 1025 / 16384 faces.

    The dominant face is not combined with 16384 faces: the others would share under 1 % of 2^24 uniforms, 2.5 each, and "every
    face the float64 inverse CDF draws once is drawn" cannot hold for any table of 32-bit entries there."""
    verts, faces = _soup(nf, variant)
    a64 = dh.face_areas_f64(verts, faces)
    a32 = dh.face_areas_f32(verts, faces)
    zero = a64 == 0
    assert np.array_equal(a32 == 0, zero), "a degenerate face is exactly zero in fp32, and only those"
    assert int(zero.sum()) >= int(round(0.1 * nf)) - (variant == "dominant") and not zero.all()
    if variant == "ends":
        assert zero[0] and zero[-1]
    if variant == "dominant":
        assert a64.max() > 0.99 * a64.sum()
    tab = dh.table(a32)
    assert tab.dtype == np.float32
    steps = np.diff(np.concatenate([[0], tab.astype(np.float64)]))
    assert (steps >= 0).all(), "the table steps down at %s" % np.flatnonzero(steps < 0)[:8]
    assert (steps[zero] == 0).all(), "a zero-area face has a step of its own: %s" % np.flatnonzero(zero & (steps != 0))[:8]
    assert abs(float(tab[-1]) / a64.sum() - 1) < 64 * dh.U

    r0 = (np.arange(dh.GRID, dtype=np.uint32).astype(np.float32) * np.float32(dh.U)).astype(np.float32)      # exact
    choices = dh.search(tab, dh.search_targets(tab, r0))
    assert not zero[choices].any(), "%d uniforms draw a zero-area face" % int(zero[choices].sum())
    assert (np.diff(choices) >= 0).all(), "the face drawn decreases with the uniform"
    counts = np.bincount(choices, minlength=nf)
    ref = dh.sweep_counts_f64(a64)
    missing = np.flatnonzero((ref > 0) & (counts == 0))
    assert missing.size == 0, "faces the float64 inverse CDF draws and the table does not: %s (float64 counts %s)" % (missing[:8], ref[missing[:8]])
    K = dh.count_bound(nf)
    worst = int(np.abs(counts - ref).max())
    print("nf %d %s: K %d, worst count difference %d" % (nf, variant, K, worst))
    assert worst <= K, "a face's count is %d from its float64 count (K = %d)" % (worst, K)


def test_literal_search_is_the_inverse_of_a_sorted_table():
    """On a non-decreasing table the kernel's loop is searchsorted(side="right") clamped to the last entry -- also on tables of one
    entry, of zeros only, and with flat runs at both ends."""
    rng = np.random.default_rng(5)
    for n in (1, 2, 3, 20, 1023, 1025):
        for tab in (np.cumsum(rng.integers(0, 4, n)).astype(np.float32), np.zeros(n, dtype=np.float32)):
            target = np.arange(0, int(tab[-1]) + 2, dtype=np.float32) - np.float32(0.5)
            assert np.array_equal(dh.search(tab, target), np.minimum(np.searchsorted(tab, target, side="right"), n - 1))
