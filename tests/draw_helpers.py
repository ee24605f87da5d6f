"""Shared by tests/test_draw_exact_host.py and tests/test_draw_exact_gpu.py: the face sampler (csrc/draw_body.h) restated on the host
operation for operation -- the Philox4x32-10 stream with the kernel's counter and key layout, the fp32 face areas, the
table the search reads, the search, the barycentric point -- and the float64 inverse CDF both are held to, with the bound of a
face's count.  Everything here is numpy; nothing needs a GPU."""
import numpy as np

THREADS, WAVE, MAX_FACES = 1024, 64, 16384      # DRAW_THREADS, GEOM_WAVE, DRAW_MAX_FACES
GRID = 1 << 24                                  # a uniform carries 24 bits: u01(x) = (x >> 8) * 2^-24
M32 = np.uint64(0xFFFFFFFF)
SEARCH_CHUNK = 1 << 16
U = 2.0 ** -24                                  # the unit round-off of binary32


# ------------------------------------------------------------------------------------------------ the random stream ----
def philox4x32_10(ctr, key):
    """Philox4x32-10 (Salmon et al. 2011, the Random123 reference): ctr [..., 4], key [..., 2] (or a pair of ints), any unsigned
    words below 2^32 -> [..., 4] uint32.  All arithmetic in uint64 (a 32 x 32 bit product fits)."""
    ctr = np.asarray(ctr, dtype=np.uint64)
    key = np.asarray(key, dtype=np.uint64)
    c0, c1, c2, c3 = (ctr[..., i] & M32 for i in range(4))
    k0, k1 = key[..., 0] & M32, key[..., 1] & M32
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c0
        p1 = np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & M32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & M32
        k0 = (k0 + np.uint64(0x9E3779B9)) & M32
        k1 = (k1 + np.uint64(0xBB67AE85)) & M32
    return np.stack([c0, c1, c2, c3], axis=-1).astype(np.uint32)


def u01(x):
    """[0, 1) from the 24 high bits of a word, as fp32 (exact)."""
    return ((np.asarray(x, dtype=np.uint32) >> np.uint32(8)).astype(np.float32) * np.float32(U)).astype(np.float32)


def stream_words(seed, position, mesh_global, num):
    """The four words of samples 0 .. num-1 of one mesh: counter = (sample, global mesh index truncated to 32 bits, low and high
    half of the stream position), key = (low, high) half of the seed."""
    ctr = np.empty((num, 4), dtype=np.uint64)
    ctr[:, 0] = np.arange(num, dtype=np.uint64)
    ctr[:, 1] = int(mesh_global) & 0xFFFFFFFF
    ctr[:, 2] = int(position) & 0xFFFFFFFF
    ctr[:, 3] = (int(position) >> 32) & 0xFFFFFFFF
    return philox4x32_10(ctr, (int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF))


def stream_uniforms(seed, position, mesh_global, num):
    """(r0, r1, r2) of samples 0 .. num-1 of one mesh, fp32 [num] each: the face uniform, U1 and U2."""
    w = stream_words(seed, position, mesh_global, num)
    return u01(w[:, 0]), u01(w[:, 1]), u01(w[:, 2])


# -------------------------------------------------------------------------------------------------- the table ----------
def face_areas_f32(verts, faces):
    """fp32 areas [nf] with the kernel's expression: x = v0 - v1, y = v1 - v2, sqrt((ca^2 + cb^2) + cc^2) / 2 (no contraction)."""
    verts = np.asarray(verts, dtype=np.float32)
    v0, v1, v2 = (verts[faces[:, k]] for k in range(3))
    with np.errstate(invalid="ignore", over="ignore"):            # (a non-finite vertex: Inf - Inf, 0 * Inf are what the kernel forms)
        x, y = v0 - v1, v1 - v2
        ca = x[:, 1] * y[:, 2] - x[:, 2] * y[:, 1]
        cb = x[:, 2] * y[:, 0] - x[:, 0] * y[:, 2]
        cc = x[:, 0] * y[:, 1] - x[:, 1] * y[:, 0]
        return (np.sqrt((ca * ca + cb * cb) + cc * cc) / np.float32(2)).astype(np.float32)


def scanned_sums_f32(weights):
    """The workgroup's fp32 inclusive sums of the weights, [nf], in the kernel's three pieces: thread t adds its `per` consecutive
    entries in order (local sums), a 64-lane Hillis-Steele scan adds the thread totals of a wave, the 16 wave totals are added in
    order into a base, and entry f = local sum + (base + (inclusive - own total)).  NOT monotone across a thread boundary."""
    nf = weights.size
    per = (nf + THREADS - 1) // THREADS
    padded = np.zeros(THREADS * per, dtype=np.float32)
    padded[:nf] = weights
    padded = padded.reshape(THREADS, per)
    local = np.empty_like(padded)
    run = np.zeros(THREADS, dtype=np.float32)
    for j in range(per):
        run = run + padded[:, j]
        local[:, j] = run
    incl = run.reshape(THREADS // WAVE, WAVE).copy()
    lanes = np.arange(WAVE)
    off = 1
    while off < WAVE:
        up = np.zeros_like(incl)
        up[:, off:] = incl[:, :-off]
        incl = np.where(lanes >= off, incl + up, incl).astype(np.float32)
        off <<= 1
    base = np.zeros(THREADS // WAVE, dtype=np.float32)
    acc = np.float32(0)
    for w in range(THREADS // WAVE):
        base[w] = acc
        acc = np.float32(acc + incl[w, WAVE - 1])
    offset = (base[:, None] + (incl - run.reshape(THREADS // WAVE, WAVE))).astype(np.float32).reshape(THREADS)
    return (local + offset[:, None]).astype(np.float32).reshape(-1)[:nf]


def weighing(areas):
    """What a face adds to the running sums: its area where `area > 0`, else 0 -- a NaN area weighs nothing, exactly like a
    zero one.  No bit changes for finite areas: a zero area added 0 before."""
    areas = np.asarray(areas, dtype=np.float32)
    return np.where(areas > 0, areas, np.float32(0)).astype(np.float32)


def table(weights, sums=None):
    """The fp32 table the search reads, [nf]: entry f = the largest scanned sum over the entries <= f that weigh something, 0 in
    front of the first.  max is exactly associative, so the order the kernel takes it in (per thread, wave scan, wave maxima)
    does not matter; it is the kernel's fmaxf, which passes over a NaN sum (an Inf area: Inf - Inf in its thread's offset).
    `sums` (the tests' planted faults): another scan than scanned_sums_f32 of what weighs."""
    weights = np.asarray(weights, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        if sums is None:
            sums = scanned_sums_f32(weighing(weights))
        steps = np.concatenate(([np.float32(0)], np.where(weights > 0, sums, np.float32(0)))).astype(np.float32)
        return np.fmax.accumulate(steps)[1:]                      # (the kernel's maximum starts from 0 in front of the first entry)


def search_targets(tab, r0):
    """target = r0 * total in fp32: below the total for r0 <= 1 - 2^-24 whenever the total is positive."""
    with np.errstate(invalid="ignore"):                           # (0 * Inf: a NaN target ends on the last face, like an Inf one)
        return (np.asarray(r0, dtype=np.float32) * tab[-1]).astype(np.float32)


def search(tab, target):
    """The kernel's binary search, literally: first f with tab[f] > target in [0, nf - 1], whatever the table holds."""
    target = np.asarray(target)
    if target.size > SEARCH_CHUNK:           # (in pieces that stay in the cache: a sweep of 2^24 targets takes half the time)
        flat = target.reshape(-1)
        out = np.empty(flat.size, dtype=np.int64)
        for s in range(0, flat.size, SEARCH_CHUNK):
            out[s:s + SEARCH_CHUNK] = search(tab, flat[s:s + SEARCH_CHUNK])
        return out.reshape(target.shape)
    lo = np.zeros(target.shape, dtype=np.int32)
    hi = np.full(target.shape, tab.size - 1, dtype=np.int32)
    for _ in range(int(tab.size - 1).bit_length() + 1):
        live = lo < hi
        if not live.any():
            break
        mid = (lo + hi) >> 1
        gt = tab[mid] > target
        hi = np.where(live & gt, mid, hi)
        lo = np.where(live & ~gt, mid + 1, lo)
    assert not (lo < hi).any()
    return lo.astype(np.int64)


def draw(verts, faces, r0, r1, r2, order=None):
    """One mesh: (choices int64, u, v, points [num, 3]) of the uniforms r0, r1, r2 (fp32 [num]) with the kernel's arithmetic.
    `order` [nf] (the visiting-order route): the table is built over the faces in that order, an entry that is no face weighs
    nothing."""
    verts = np.asarray(verts, dtype=np.float32)
    areas = face_areas_f32(verts, faces)
    if order is not None:
        real = (order >= 0) & (order < faces.shape[0])
        areas = np.where(real, areas[np.where(real, order, 0)], np.float32(0)).astype(np.float32)
    tab = table(areas)
    slot = search(tab, search_targets(tab, r0))
    choices = slot if order is None else np.where(real[slot], order[slot], 0).astype(np.int64)
    su = np.sqrt(np.asarray(r1, dtype=np.float32))
    v = np.asarray(r2, dtype=np.float32)
    return choices, su, v, sampled_points(verts, faces, choices, su, v)


def sampled_points(verts, faces, choices, su, v):
    """((1 - u) x + (u (1 - v)) y) + (u v) z in fp32, the kernel's (and the reference's) evaluation order: [num, 3]."""
    x, y, z = (np.asarray(verts, dtype=np.float32)[faces[choices, k]] for k in range(3))
    one = np.float32(1)
    w0, w1, w2 = one - su, su * (one - v), su * v
    with np.errstate(invalid="ignore"):
        return ((x * w0[:, None] + y * w1[:, None]) + z * w2[:, None]).astype(np.float32)


# ------------------------------------------------------------------------------------ the float64 reference and its bound ----
def face_areas_f64(verts, faces):
    """float64 areas [nf] of the fp32 vertices."""
    v = np.asarray(verts, dtype=np.float32).astype(np.float64)
    return np.linalg.norm(np.cross(v[faces[:, 0]] - v[faces[:, 1]], v[faces[:, 1]] - v[faces[:, 2]]), axis=1) / 2


def inverse_cdf_f64(areas64, r0):
    """The reference: face = searchsorted(cumsum(areas), r0 * total, side="right"), clamped to the last face."""
    cum = np.cumsum(areas64)
    return np.minimum(np.searchsorted(cum, np.asarray(r0, dtype=np.float64) * cum[-1], side="right"), areas64.size - 1)


def sweep_counts_f64(areas64):
    """Per-face counts of the reference over the uniforms k / 2^24, k = 0 .. 2^24 - 1."""
    r0 = np.arange(GRID, dtype=np.float64) / GRID
    return np.bincount(inverse_cdf_f64(areas64, r0), minlength=areas64.size)


def count_bound(nf):
    """K: how far a face's count over the 2^24 uniforms may lie from the float64 count.  A face's count is the number of grid
    points of 2^-24 between its two boundaries, and a boundary is displaced by at most one grid point per fp32 rounding on the way
    to its table entry (a rounding is at most u = 2^-24 of a partial sum, itself at most the total): per - 1 local additions and
    the offset's (counted as `per`), 6 steps of the wave scan, 15 additions of wave totals, and 8 for the area's own expression
    (three differences, two products and a difference per component, squares, two sums, root).  The running maximum adds none:
    it is the sum of an entry at or in front of f, which lies no further above the exact sum at f than its own rounding, and no
    further below than that of the last entry that weighs something.  K = 2 * (per + 6 + 15 + 8): 60 at one face a thread, 90
    at sixteen."""
    return 2 * ((nf + THREADS - 1) // THREADS + 6 + 15 + 8)


# ------------------------------------------------------------------------------------------------- the meshes ----------
def triangle_soup(nf, seed, variant="plain"):
    """(verts fp32 [nv, 3], faces int64 [nf, 3]): vertices 0.5 * N(0, 1), random corner triples of three different vertices, one
    face in ten degenerate by a repeated corner (exactly zero area in fp32).  variant "ends": the first and the last face are
    degenerate too; "dominant": face nf // 3 gets three vertices of its own, far apart -- more than 99 % of the area."""
    rng = np.random.default_rng(seed)
    nv = max(8, nf // 2)
    verts = (0.5 * rng.standard_normal((nv, 3))).astype(np.float32)
    faces = np.empty((nf, 3), dtype=np.int64)
    for f in range(nf):
        faces[f] = rng.choice(nv, 3, replace=False)
    degenerate = rng.choice(nf, int(round(0.1 * nf)), replace=False)
    if variant == "ends":
        degenerate = np.union1d(degenerate, [0, nf - 1])
    faces[degenerate, 2] = faces[degenerate, 0]
    if variant == "dominant":
        big = (10.0 * np.sqrt(nf) * rng.standard_normal((3, 3))).astype(np.float32)     # ~ 400 x the area of all the others
        verts = np.concatenate([verts, big])
        faces[nf // 3] = [nv, nv + 1, nv + 2]
    return verts, faces
