"""Skins, poses and expectations of the skinning tests (rt_set_skin / rt_pose_skin* / rt_skin_vertices).

The expectations are numpy's alone: `rule32` restates the rule of include/rtx_amd.h in elementwise
np.float32 arithmetic, one rounding per operation and nothing fused; `rule64` evaluates the same sums in
float64, with the magnitude sum the error bound needs.  Neither calls the library."""
import numpy as np

F = np.float32


def rule32(rest, joints, weights, matrices):
    """The rule in float32: acc = +0; for k = 0..3: acc = acc + w_k * (((m0 px + m1 py) + m2 pz) + m3), an
    influence of weight 0 leaving acc as it is (its matrix is gathered here, but never used)."""
    rest = np.asarray(rest, F)
    m = np.asarray(matrices, F).reshape(-1, 3, 4)
    px, py, pz = rest[:, 0:1], rest[:, 1:2], rest[:, 2:3]
    acc = np.zeros((len(rest), 3), F)
    with np.errstate(all="ignore"):
        for k in range(4):
            mk = m[joints[:, k].astype(np.int64)]  # (nv, 3, 4)
            t = ((mk[:, :, 0] * px + mk[:, :, 1] * py) + mk[:, :, 2] * pz) + mk[:, :, 3]
            w = weights[:, k:k + 1].astype(F)
            assert t.dtype == F and w.dtype == F
            acc = np.where(w == 0, acc, acc + w * t)
    assert acc.dtype == F
    return acc


def rule64(rest, joints, weights, matrices):
    """(the rule's sums in float64, the magnitude sums  sum_k |w_k| (|M_k| |(p, 1)|)_r  in float64)."""
    p = np.concatenate([np.asarray(rest, np.float64), np.ones((len(rest), 1))], axis=1)  # (nv, 4)
    m = np.asarray(matrices, np.float64).reshape(-1, 3, 4)
    out = np.zeros((len(rest), 3))
    mag = np.zeros((len(rest), 3))
    for k in range(4):
        mk = m[joints[:, k].astype(np.int64)]
        w = weights[:, k:k + 1].astype(np.float64)
        out += w * np.einsum("vrc,vc->vr", mk, p)
        mag += np.abs(w) * np.einsum("vrc,vc->vr", np.abs(mk), np.abs(p))
    return out, mag


def identity(nj):
    m = np.zeros((nj, 3, 4), F)
    m[:, 0, 0] = m[:, 1, 1] = m[:, 2, 2] = 1
    return m


def rotation(axis, angle, pivot=(0.0, 0.0, 0.0)):
    """(3, 4): a rotation by `angle` about the unit `axis` through `pivot` (Rodrigues, in float64, rounded once)."""
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    R = np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)
    c = np.asarray(pivot, np.float64)
    return np.concatenate([R, (c - R @ c)[:, None]], axis=1).astype(F)


def translation(offset):
    m = identity(1)[0]
    m[:, 3] = np.asarray(offset, F)
    return m


def scale(sx, sy, sz):
    m = np.zeros((3, 4), F)
    m[0, 0], m[1, 1], m[2, 2] = sx, sy, sz
    return m


def random_pose(nj, seed, amount=1.0):
    """nj matrices: rotations about seeded axes through seeded pivots, with a translation; every fourth a
    non-uniform scale times its rotation."""
    rng = np.random.default_rng(seed)
    out = np.zeros((nj, 3, 4), F)
    for j in range(nj):
        m = rotation(rng.normal(size=3) + 1e-3, amount * rng.uniform(-0.6, 0.6), rng.uniform(-2, 6, size=3)).astype(np.float64)
        m[:, 3] += amount * rng.uniform(-0.3, 0.3, size=3)
        if j % 4 == 3:
            m = np.diag(1.0 + amount * rng.uniform(-0.2, 0.2, size=3)) @ m
        out[j] = m.astype(F)
    return out


def random_skin(nv, nj, seed, rest=None, last_joint=True):
    """(rest, joints, weights): seeded rest positions unless given; vertex v has 1 + v % 4 non-zero weights,
    in slots that rotate with v so that every slot pattern of 1..4 occurs; the weights of a vertex sum to
    about 1 without being normalised; zero-weight slots name valid joints too.  last_joint: some vertex
    names joint nj - 1 with a non-zero weight."""
    rng = np.random.default_rng(seed)
    if rest is None:
        rest = rng.uniform(-4, 4, size=(nv, 3)).astype(F)
    joints = rng.integers(0, nj, size=(nv, 4)).astype(np.uint16)
    weights = np.zeros((nv, 4), F)
    for v in range(nv):
        cnt = 1 + v % 4
        slots = [(v // 4 + s) % 4 for s in range(cnt)]
        w = rng.uniform(0.1, 1.0, size=cnt)
        weights[v, slots] = (w / w.sum()).astype(F)
    if last_joint:
        v = nv // 2
        k = int(np.nonzero(weights[v])[0][0])
        joints[v, k] = nj - 1
    return np.ascontiguousarray(rest, F), joints, weights


def slot_patterns(weights):
    """The set of non-zero slot masks (bit k: slot k) among the vertices."""
    return set(int(x) for x in ((weights != 0) * (1 << np.arange(4))).sum(1))
