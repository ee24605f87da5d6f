"""Shared by tests/test_face_split_gpu.py and tests/test_face_split_host.py: the fixtures of tests/golden/make_face_split.py taken
apart, and the float64 restatements of the face-splitting kernels (csrc/face_split.hip) with the bound of every element."""
import functools

import numpy as np

import helpers

U = 2.0 ** -24                 # the unit round-off of binary32
ICO_CASES = ("split_ico1_threshold", "split_ico1_fallback", "split_ico1_two_rounds", "split_ico2_two_rounds")
POLE_LISTS = ("pole", "two", "all")
C_FIXTURE = 5


@functools.lru_cache(maxsize=None)
def fixture(name):
    return helpers.golden(name)


def fixture_rounds(name):
    """The rounds of an icosphere case, each a dict without its `rN.` prefix."""
    g = fixture(name)
    return [{k[3:]: v for k, v in g.items() if k.startswith("r%d." % r)} for r in range(1, int(g["rounds"]) + 1)]


def pole_lists():
    """The three hand-made lists of split_482_pole, each a dict without its prefix and with the inputs they share."""
    g = fixture("split_482_pole")
    shared = {k[5:]: v for k, v in g.items() if k.startswith("pole.in.")}
    out = {}
    for name in POLE_LISTS:
        d = {k[len(name) + 1:]: v for k, v in g.items() if k.startswith(name + ".")}
        d.update(shared)
        out[name] = d
    return out, int(g["pole_vertex"])


def dense(rnd, values=True):
    """The dense fp32 matrix of a round's adjacency fixture: `adj` (values) or `adj_orig` (ones at the same places)."""
    n = int(rnd["nv"])
    m = np.zeros((n, n), np.float32)
    m[rnd["adj.rows"].astype(np.int64), rnd["adj.cols"].astype(np.int64)] = rnd["adj.vals"] if values else 1.0
    return m


def grad_out(rnd):
    """The seeded cotangent of a round's (verts, features), as the generator drew it."""
    seed = int(rnd["grad_seed"])
    return helpers.seeded_input([seed, 2], rnd["verts"].shape), helpers.seeded_input([seed, 3], rnd["features"].shape)


# ---- curvature ---------------------------------------------------------------------------------------------------------------
def _normals64(v, f):
    p1, p2, p3 = v[f[:, 1]], v[f[:, 0]], v[f[:, 2]]
    e1, e2 = p2 - p1, p3 - p1
    raw = np.cross(e1, e2)
    with np.errstate(all="ignore"):
        length = np.linalg.norm(raw, axis=1)
        kappa = np.linalg.norm(e1, axis=1) * np.linalg.norm(e2, axis=1) / length        # 1 / sin(angle between the edges)
        return raw / length[:, None], kappa


def curvature64(verts, faces, face_list):
    """(curvature [Fa] in radians, bound [Fa]): geom_face_curvature_f32 restated in float64 with the bound of each element.

    The chain of one neighbour term, u = 2^-24, first order:
      * an edge vector is one fp32 subtraction of exact inputs (u); a component a*b - c*d of the cross product carries 2u + u per
        product and u for the difference: <= 4u (|ab| + |cd|) <= 4u |e1||e2|, so the raw normal is off by at most 4 sqrt(3) u
        |e1||e2| -- 4 sqrt(3) u kappa of its own length, kappa = |e1||e2| / |e1 x e2| (a sliver face is ill-conditioned and its
        bound says so);
      * the length (3 squares, 2 sums, a root: <= 3.5u) and the division (u) rescale the normal: <= 4.5u along it;
      * the dot product of two unit vectors: 3 products and 2 sums, <= 3u.
    So the cosine is off by at most k u with  k = 4 sqrt(3) (kappa_own + kappa_neighbour) + 2 * 4.5 + 3 = 4 sqrt(3) (kappa_own +
    kappa_neighbour) + 12,  and the term by k u / sqrt(1 - c^2), the derivative of acos taken at the clamped cosine moved k u
    towards the clamp (where it reaches ~224: a flat tolerance would be wrong), plus 2 ulps of acosf's own result.  The mean adds
    two sums and a division: 3u of the result."""
    v, f, fl = np.asarray(verts, np.float64), np.asarray(faces, np.int64), np.asarray(face_list, np.int64)
    n, kappa = _normals64(v, f)
    own = fl[:, 0, 2]
    eps = np.float64(np.float32(.00001))
    total, bound = np.zeros(len(fl)), np.zeros(len(fl))
    with np.errstate(all="ignore"):
        for j in range(3):
            nb = fl[:, j, 0]
            c = np.clip((n[own] * n[nb]).sum(1), -1.0 + eps, 1.0 - eps)
            k = 4.0 * np.sqrt(3.0) * (kappa[own] + kappa[nb]) + 12.0
            worst_c = np.minimum(np.abs(c) + k * U, 1.0 - eps)
            term = np.arccos(c)
            total += term
            bound += k * U / np.sqrt(1.0 - worst_c ** 2) + 2.0 * U * term
    curv = total / 3.0
    return curv, bound / 3.0 + 3.0 * U * curv


def curvature32_host(verts, faces, face_list, neighbour_slots=(0, 1, 2), clamp=True):
    """The same formulas in plain fp32 torch on the host, the reference's operations in its order (old_GEOMetrics/utils.py:
    437-465).  neighbour_slots / clamp plant the two faults the bound has to catch: a wrong neighbour slot, an unclamped cosine."""
    import torch
    v, f, fl = torch.as_tensor(verts, dtype=torch.float32), torch.as_tensor(faces).long(), torch.as_tensor(face_list).long()
    p1, p2, p3 = v[f[:, 1]], v[f[:, 0]], v[f[:, 2]]
    normals = torch.cross(p2 - p1, p3 - p1, dim=1)
    normals = normals / torch.norm(normals, p=2, dim=1).view(-1, 1)
    own = normals[fl[:, 0, 2]]
    terms = []
    for j in neighbour_slots:
        c = torch.sum(own * normals[fl[:, j, 0]], dim=1)
        if clamp:
            c = c.clamp(-1.0 + .00001, 1.0 - .00001)
        terms.append(c.acos().view(-1, 1))
    return torch.mean(torch.cat(terms, dim=1), dim=1).numpy()


def curvature_close(got, exact, bound, what, share=1.0):
    """(|got - exact| <= share * bound on every face with a curvature and NaN exactly where the restatement has NaN, the worst
    element as a share of its bound -- inf for a NaN out of place)."""
    got = np.asarray(got, np.float64)
    if not (np.isnan(got) == np.isnan(exact)).all():
        return False, float("inf")
    ok = ~np.isnan(exact)
    worst = float((np.abs(got - exact)[ok] / bound[ok]).max())
    return worst <= share, worst


# ---- the vertices' split and its transpose -----------------------------------------------------------------------------------
def corners_of(rnd):
    """[S,3] vertex ids of the faces a round splits, in the order of its `splitting`."""
    own = rnd["in.face_list"][rnd["splitting"], 0, 2]
    return rnd["in.faces"][own]


def new_rows32(x, corners):
    """(x/3 + y/3) + z/3 in fp32 with true divisions: what the reference's expression rounds to (utils.py:595)."""
    x = np.asarray(x, np.float32)
    three = np.float32(3.0)
    return (x[corners[:, 0]] / three + x[corners[:, 1]] / three) + x[corners[:, 2]] / three


def split_transpose64(g, corners, nv):
    """The transpose of the vertices' split in float64: (exact [nv,C], mass [nv,C], deg_split [nv]) with
    exact[u] = g[u] + sum_{s: u corner of s} g[nv + s] / 3, mass the same with absolute values."""
    g = np.asarray(g, np.float64)
    exact, mass = g[:nv].copy(), np.abs(g[:nv])
    deg = np.zeros(nv, np.int64)
    for k in range(3):
        np.add.at(exact, corners[:, k], g[nv:] / 3.0)
        np.add.at(mass, corners[:, k], np.abs(g[nv:]) / 3.0)
        np.add.at(deg, corners[:, k], 1)
    return exact, mass, deg


def split_gradient_close(got, g, corners, nv, what):
    """Every element of an input gradient of the split within (deg_split(u) + 1 + 2) * 2^-24 of its terms' mass: deg_split(u)
    additions, one division per term, and the project's allowance of 2."""
    exact, mass, deg = split_transpose64(g, corners, nv)
    return helpers.rows_close(got, exact, mass * ((deg + 3) * U)[:, None], 1.0, what)


# ---- the tables of a split restated in numpy (the reference cannot split ONE face: its indexing with a one-element tensor
# drops a dimension, old_GEOMetrics/utils.py:580-587; this restatement reproduces every fixture and then serves S = 1) ---------------
def split_tables_restated(faces, face_list, splitting, adj_orig):
    """(faces [Ft+3S,3], face_list [Fa+2S,3,3], adj fp32 [V+S,V+S], adj_orig) after splitting the active rows `splitting`, by the
    rules of the reference's split_info written out row by row."""
    faces, fl, sp = np.asarray(faces, np.int64), np.asarray(face_list, np.int64), np.asarray(splitting, np.int64)
    nv, nft, nfa, s = adj_orig.shape[0], len(faces), len(fl), len(sp)
    own = fl[sp, 0, 2]
    corners = faces[own]
    face_s = np.full(nft, -1, np.int64)
    face_s[own] = np.arange(s)
    split_pos = np.full(nfa, -1, np.int64)
    split_pos[sp] = np.arange(s)
    new_vertex = nv + np.arange(s)
    x, y, z = corners[:, 0], corners[:, 1], corners[:, 2]
    new_faces = np.concatenate((faces, np.stack((x, y, new_vertex), 1), np.stack((new_vertex, y, z), 1), np.stack((x, new_vertex, z), 1)))

    def across(row, j):          # a split neighbour is replaced by its child with the same edge label
        f, label = row[j, 0], row[j, 1]
        return nft + label * s + face_s[f] if face_s[f] >= 0 else f
    kept, children = [], [[], [], []]
    for i in range(nfa):
        row = fl[i]
        if split_pos[i] < 0:
            kept.append([[across(row, j), row[j, 1], row[0, 2]] for j in range(3)])
    for k in range(s):
        row = fl[sp[k]]
        c = [nft + m * s + k for m in range(3)]
        for m in range(3):
            children[m].append([[across(row, j), row[j, 1], c[m]] if j == m else [c[j], m, c[m]] for j in range(3)])
    new_fl = np.array(kept + children[0] + children[1] + children[2], np.int64).reshape(nfa + 2 * s, 3, 3)
    n = nv + s
    new_orig = np.zeros((n, n), np.float32)
    new_orig[:nv, :nv] = adj_orig
    for k in range(3):
        new_orig[new_vertex, corners[:, k]] = 1
        new_orig[corners[:, k], new_vertex] = 1
    new_orig[new_vertex, new_vertex] = 1
    adj = new_orig * (np.float32(1.0) / new_orig.sum(1, dtype=np.float32))[:, None]
    return new_faces, new_fl, adj, new_orig
