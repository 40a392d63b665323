"""GPU parity of the HIP skinning kernels (csrc/skinning.hip) where an eigen-decomposition of F^T F can go wrong and an SVD of F
cannot: planar, thin, needle-like, mirrored, collapsed and isotropic bone neighbourhoods (k_bone_fit); the per-environment, per-call
identity fallback; the launch geometry of k_skin / k_skin_quat; every branch of rotmat_to_quat.

The yardstick is the pinned numpy oracle (oracle/lbs_oracle.py: float32 F, float64 SVD).  All inputs are generated here from fixed seeds.

Gate on a rotation (section 1).  F is a float32 sum; on an ill-conditioned neighbourhood one ulp of that sum turns R by about
eps32 * s0 / (s1 +- s2), and the kernel adds the eight products in another order than the oracle's einsum.  So the gate is not one
number: per bone, the oracle's R is computed from F summed three ways (float32 k ascending, float32 k descending, float64; the
rotations kept in float64), `spread` is the largest difference among the three, and the kernel is held to 4 * spread + 2e-7 — 4 because
its order is a fourth draw from the same rounding population, 2e-7 for the float32 cast of R on either side.  No bone is excluded.
"""
import functools

import numpy as np
import pytest
from util_parity import close, record

pytestmark = pytest.mark.gpu

W_BASE = np.array([0.3, -0.2, 0.5])


# ---------------------------------------------------------------------------------------------------------------------------------
# inputs
def _blob(rng, n, half=0.05):
    return rng.uniform(-half, half, (n, 3)).astype(np.float32)


def _grid(rng):
    """Jittered 32 x 16 grid, 5 mm pitch, z = 0."""
    gx, gy = np.meshgrid(np.arange(32), np.arange(16), indexing="ij")
    b = np.stack([gx.ravel() * 0.005, gy.ravel() * 0.005, np.zeros(512)], -1)
    b[:, :2] += rng.uniform(-0.001, 0.001, (512, 2))
    return b.astype(np.float32)


def _axis_angle(axis, deg):
    a = np.asarray(axis, np.float64); a = a / np.linalg.norm(a)
    t = np.deg2rad(deg)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * (K @ K)


GEOMETRIES = ["plane_exact", "plane_noisy_motion", "plate_1e-6", "plate_1e-4", "needle", "mirror", "collapse", "noise", "isotropic",
              "isotropic_bcc"]


def geometry(name):
    """(bones [N,3], motions [N,3]) float32 of one section-1 case."""
    rng = np.random.default_rng(1000 + GEOMETRIES.index(name))
    base = lambda b: np.cross(W_BASE, b.astype(np.float64)) + rng.normal(0, 5e-4, b.shape)  # noqa: E731
    if name == "plane_exact":
        b = _grid(rng); m = np.cross(W_BASE, b.astype(np.float64))
    elif name == "plane_noisy_motion":
        b = _grid(rng); m = base(b)
    elif name in ("plate_1e-6", "plate_1e-4"):
        b = _grid(rng); b[:, 2] = rng.normal(0, float(name[6:]), 512); m = base(b)
    elif name == "needle":
        b = np.stack([0.002 * np.arange(512), rng.normal(0, 2e-5, 512), rng.normal(0, 2e-5, 512)], -1).astype(np.float32); m = base(b)
    elif name == "mirror":
        b = _blob(rng, 512); m = b.astype(np.float64) * np.array([0.0, 0.0, -2.0]) + rng.normal(0, 5e-4, b.shape)
    elif name == "collapse":
        b = _blob(rng, 512); m = b.astype(np.float64) * np.array([0.0, 0.0, -1.0])
    elif name == "noise":
        b = _blob(rng, 512); m = rng.normal(0, 0.02, b.shape)
    elif name == "isotropic":       # simple cubic 8^3: six axis neighbours + two face diagonals -> pairs of equal singular values
        g = np.stack(np.meshgrid(*[np.arange(8)] * 3, indexing="ij"), -1).reshape(-1, 3)
        b = (g * 0.0078125).astype(np.float32); m = b.astype(np.float64) @ (_axis_angle([1, 2, 3], np.rad2deg(0.7)) - np.eye(3)).T
    elif name == "isotropic_bcc":   # body-centred cubic: the eight nearest neighbours are (+-h, +-h, +-h) -> s0 = s1 = s2 off the boundary
        c = np.stack(np.meshgrid(*[np.arange(6)] * 3, indexing="ij"), -1).reshape(-1, 3) * 2
        i = np.stack(np.meshgrid(*[np.arange(5)] * 3, indexing="ij"), -1).reshape(-1, 3) * 2 + 1
        g = np.concatenate([c, i])                                      # 216 corners + 125 centres
        b = (g * 0.00390625).astype(np.float32); m = b.astype(np.float64) @ (_axis_angle([1, 2, 3], np.rad2deg(0.7)) - np.eye(3)).T
    return np.ascontiguousarray(b, np.float32), np.ascontiguousarray(m, np.float32)


def _points(rng, bones, P, sigma=0.003):
    return (bones[rng.integers(0, len(bones), P)] + rng.normal(0, sigma, (P, 3))).astype(np.float32)


def _weights(bones, pts, k):
    """Inverse-distance weights over the k nearest bones, like lbs_oracle.knn_weights (which cannot do k = 1)."""
    from scipy.spatial import cKDTree

    _, idx = cKDTree(bones.astype(np.float64)).query(pts.astype(np.float64), k=k)
    idx = idx.reshape(len(pts), k)
    w = (1.0 / (np.linalg.norm(bones[idx] - pts[:, None], axis=-1).astype(np.float32) + np.float32(1e-6))).astype(np.float32)
    return np.ascontiguousarray(w / w.sum(-1, keepdims=True), np.float32), np.ascontiguousarray(idx, np.int32)


def _cuda(a):
    import torch

    return torch.from_numpy(np.array(a)).cuda()   # a copy: the shared inputs are read-only


def oracle_spread(bones, motions, rel):
    """Per-bone largest difference among the oracle's float64 rotations from F summed three ways; every variant must keep rank >= 2."""
    from oracle import lbs_oracle

    Rs = []
    for how in ("f32_ascending", "f32_descending", "f64"):
        R, rank = lbs_oracle.bone_rotations(bones, motions, rel, F=lbs_oracle.fit_matrices(bones, motions, rel, how), dtype=np.float64)
        assert rank.min() >= 2, (how, int(rank.min()))
        Rs.append(R)
    d = [np.abs(Rs[i] - Rs[j]).max((1, 2)) for i, j in ((0, 1), (0, 2), (1, 2))]
    return np.maximum(np.maximum(d[0], d[1]), d[2])


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. rotation of each bone against a float64 SVD, geometry by geometry
@pytest.mark.parametrize("name", GEOMETRIES)
def test_bone_rotation_matches_svd_on_degenerate_geometry(name):
    from oracle import lbs_oracle
    from r2s_hip.skinning import Skinning

    bones, mot = geometry(name)
    N, P = len(bones), 2048
    assert N == (341 if name == "isotropic_bcc" else 512)
    rel = lbs_oracle.knn_relations(bones, 8)
    xyz = _points(np.random.default_rng(50), bones, P)
    w, wi = _weights(bones, xyz, 16)
    R_ref, rank = lbs_oracle.bone_rotations(bones, mot, rel)
    assert rank.min() >= 2
    spread = oracle_spread(bones, mot, rel)
    gate = 4.0 * spread + 2e-7

    sk = Skinning(rel, w, wi, device="cuda:0")
    out = sk.interpolate_motions(_cuda(bones), _cuda(mot), _cuda(xyz)).cpu().numpy()
    R, flags = sk.debug(1)
    R = R.cpu().numpy()[0].astype(np.float64)
    err = np.abs(R - R_ref.astype(np.float64)).max((1, 2))
    worst = int(np.argmax(err - gate))
    S = np.linalg.svd(lbs_oracle.fit_matrices(bones, mot, rel, "f64"), compute_uv=False)
    record(f"R[{name}]", oracle_spread=float(spread.max()), max_abs_err=float(err.max()), gate_at_worst_bone=float(gate[worst]),
           err_at_worst_bone=float(err[worst]), worst_margin=float((err - gate).max()), min_s1_over_s0=float((S[:, 1] / S[:, 0]).min()),
           min_s2_over_s0=float((S[:, 2] / S[:, 0]).min()), bones=N, bones_compared=int(err.size), rank2=int((rank == 2).sum()),
           det_negative=int((np.linalg.det(lbs_oracle.fit_matrices(bones, mot, rel, "f64")) < 0).sum()))
    print(f"{name}: spread {spread.max():.3e}  kernel err {err.max():.3e}  worst bone {worst}: err {err[worst]:.3e} gate {gate[worst]:.3e}")
    assert flags.cpu().numpy().tolist() == [0]
    assert np.isfinite(R).all()
    assert np.abs(np.linalg.det(R) - 1.0).max() < 1e-5 and np.abs(R @ R.transpose(0, 2, 1) - np.eye(3)).max() < 1e-5
    assert (err <= gate).all(), (name, worst, float(err[worst]), float(gate[worst]))

    ref = lbs_oracle.interpolate_motions(bones, mot, rel, xyz, w, wi)
    tol = 3e-6
    if name == "needle":  # an R error times a 3 mm offset can eat 3e-6 there
        tol = float(gate.max()) * float(np.abs(xyz[:, None] - bones[wi]).max()) + 3e-6
    assert close(out, ref, tol, what=f"xyz[{name}]")


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. the identity fallback is per environment and per call
def _flag_scene():
    from oracle import lbs_oracle

    rng = np.random.default_rng(21)
    N, P = 400, 1500
    # positions on a 2^-16 m lattice and motions on it too: every sum and difference below is exact in float32
    q = lambda a: (np.round(np.asarray(a, np.float64) * 65536.0) / 65536.0).astype(np.float32)  # noqa: E731
    bones0 = q(_blob(rng, N))
    rel = lbs_oracle.knn_relations(bones0, 8)
    xyz = _points(rng, bones0, P)
    w, wi = _weights(bones0, xyz, 16)
    motion = lambda: q(np.cross(rng.normal(0, 0.5, 3), bones0.astype(np.float64)) + rng.normal(0, 0.002, bones0.shape))  # noqa: E731
    healthy = [(q(bones0 + rng.normal(0, 1e-4, bones0.shape)), motion()) for _ in range(5)]
    victim = int(np.argmin(np.abs(bones0).sum(1)))                     # a bone in the middle of the blob
    # rank 1: the victim's 8 neighbours on the x axis through it -> F has one non-zero column, s1 = s2 = 0 exactly
    b1 = bones0.copy()
    b1[rel[victim]] = b1[victim] + np.stack([q(np.linspace(-0.01, 0.01, 8) + 0.00125), np.zeros(8), np.zeros(8)], -1).astype(np.float32)
    rank1 = (b1, motion())
    # rank 0: the victim's 8 neighbours land on the victim -> every a'_k = 0, F = 0
    m0 = motion()
    m0[rel[victim]] = (bones0[victim] + m0[victim]) - bones0[rel[victim]]
    rank0 = (bones0.copy(), m0)
    return dict(rel=rel, xyz=xyz, w=w, wi=wi, healthy=healthy, rank1=rank1, rank0=rank0, victim=victim)


def test_identity_fallback_is_per_environment_and_per_call():
    from oracle import lbs_oracle
    from r2s_hip.skinning import Skinning

    s = _flag_scene()
    rel, xyz, w, wi, victim = s["rel"], s["xyz"], s["w"], s["wi"], s["victim"]
    ident = np.tile(np.eye(3, dtype=np.float32), (len(rel), 1, 1))
    # preconditions, on the CPU: exactly one bone of the rank-1 / rank-0 environment is below rank 2, clear of the rank tolerance
    for key, want in (("rank1", 1), ("rank0", 0)):
        b, m = s[key]
        F = lbs_oracle.fit_matrices(b, m, rel, "f32_ascending")
        S = np.linalg.svd(F.astype(np.float64), compute_uv=False)
        rank = (S > 3 * lbs_oracle.EPS32 * S[:, :1]).sum(1)
        assert rank[victim] == want and (np.delete(rank, victim) >= 2).all() and not F[victim][:, want:].any()
        assert (np.delete(S[:, 1], victim) > 1e-3 * np.delete(S[:, 0], victim)).all()
        Ro, _ = lbs_oracle.bone_rotations(b, m, rel)
        assert np.array_equal(Ro, ident)
    assert not np.abs(lbs_oracle.bone_offsets(*s["rank0"], rel)[1][victim]).any()
    for b, m in s["healthy"]:
        assert lbs_oracle.bone_rotations(b, m, rel)[1].min() >= 2

    sk = Skinning(rel, w, wi, device="cuda:0")

    def run(envs, want_flags, tag):
        b = np.stack([e[0] for e in envs]); m = np.stack([e[1] for e in envs])
        out = sk.interpolate_motions(_cuda(b), _cuda(m), _cuda(np.stack([xyz] * len(envs)))).cpu().numpy()
        R, flags = sk.debug(len(envs))
        assert flags.cpu().numpy().tolist() == want_flags, tag
        assert np.isfinite(out).all(), tag
        R = R.cpu().numpy()
        for e, (be, me) in enumerate(envs):
            Ro, _ = lbs_oracle.bone_rotations(be, me, rel)
            assert np.array_equal(Ro, ident) == bool(want_flags[e])
            if not want_flags[e]:   # rotations applied
                assert np.abs(R[e].astype(np.float64) - Ro).max() < 1e-5, (tag, e)
                assert np.abs(Ro - ident).max() > 1e-2
            assert close(out[e], lbs_oracle.interpolate_motions(be, me, rel, xyz, w, wi), 3e-6, what=f"flags {tag} env {e}"), (tag, e)

    h = s["healthy"]
    run([h[0], s["rank1"], h[1]], [0, 1, 0], "rank 1 in env 1")
    run([h[2], h[3], h[4]], [0, 0, 0], "same object, healthy")          # a surviving flag would freeze env 1's rotations
    run([s["rank0"], h[0]], [1, 0], "rank 0 in env 0")
    run([h[1], h[2]], [0, 0], "healthy again")


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. k_skin / k_skin_quat launch geometry
N3, E3MAX, P3MAX, K3MAX = 300, 17, 1000, 19


@functools.lru_cache(maxsize=None)
def _scene3():
    """One blob topology; 17 environments with their own bones and motions; 1000 points with their 19 nearest bones."""
    from oracle import lbs_oracle
    from scipy.spatial import cKDTree

    rng = np.random.default_rng(33)
    bones0 = _blob(rng, N3)
    rel = lbs_oracle.knn_relations(bones0, 8)
    bones = np.stack([bones0 + rng.normal(0, 1e-4, bones0.shape).astype(np.float32) for _ in range(E3MAX)])
    mot = np.stack([np.cross(rng.normal(0, 0.5, 3), bones0) + rng.normal(0, 0.002, bones0.shape) for _ in range(E3MAX)]).astype(np.float32)
    xyz0 = _points(rng, bones0, P3MAX)
    xyz = np.stack([xyz0 + rng.normal(0, 2e-4, xyz0.shape).astype(np.float32) for _ in range(E3MAX)])
    _, idx = cKDTree(bones0.astype(np.float64)).query(xyz0.astype(np.float64), k=K3MAX)
    dist = np.linalg.norm(bones0[idx] - xyz0[:, None], axis=-1).astype(np.float32)
    quat = rng.normal(0, 1, (E3MAX, P3MAX, 4)); quat = (quat / np.linalg.norm(quat, axis=-1, keepdims=True)).astype(np.float32)
    for a in (rel, bones, mot, xyz, idx, dist, quat):
        a.setflags(write=False)
    return dict(rel=rel, bones=bones, mot=mot, xyz=xyz, idx=idx.astype(np.int32), dist=dist, quat=quat)


@functools.lru_cache(maxsize=None)
def _weights3(P, k):
    s = _scene3()
    w = (1.0 / (s["dist"][:P, :k] + np.float32(1e-6))).astype(np.float32)
    return np.ascontiguousarray(w / w.sum(-1, keepdims=True), np.float32), np.ascontiguousarray(s["idx"][:P, :k])


@functools.lru_cache(maxsize=None)
def _ref3(e, P, k):
    from oracle import lbs_oracle

    s = _scene3(); w, wi = _weights3(P, k)
    ref = lbs_oracle.interpolate_motions(s["bones"][e], s["mot"][e], s["rel"], s["xyz"][e, :P], w, wi)
    ref.setflags(write=False)
    return ref


@functools.lru_cache(maxsize=None)
def _refq3(e, P, k):
    from oracle import lbs_oracle

    s = _scene3(); w, wi = _weights3(P, k)
    ref = lbs_oracle.rotate_quats(s["bones"][e], s["mot"][e], s["rel"], s["quat"][e, :P], w, wi)
    ref.setflags(write=False)
    return ref


def _check_skin(E, P, k, variant="plain"):
    import torch
    from r2s_hip.skinning import Skinning

    s = _scene3(); w, wi = _weights3(P, k)
    sk = Skinning(s["rel"], w, wi, device="cuda:0")
    b, m = _cuda(s["bones"][:E]), _cuda(s["mot"][:E])
    x = _cuda(s["xyz"][:E, :P])
    alone = torch.stack([sk.interpolate_motions(b[e:e + 1], m[e:e + 1], x[e:e + 1])[0] for e in range(E)]).cpu().numpy()  # each as E = 1
    pad = None
    if variant == "plain":
        out = sk.interpolate_motions(b, m, x)
    elif variant == "inplace":
        buf = x.clone()
        out = sk.interpolate_motions(b, m, buf, out=buf)
        assert out.data_ptr() == buf.data_ptr()
    else:  # row-prefix views of [E, P + 37, 3] buffers: environment stride 3 (P + 37)
        g = torch.Generator().manual_seed(5)
        bin_ = torch.rand(E, P + 37, 3, generator=g).cuda(); bin_[:, :P] = x
        bout = bin_ if variant == "strided_inplace" else torch.rand(E, P + 37, 3, generator=g).cuda()
        pad = [(t, t[:, P:].clone()) for t in {id(bin_): bin_, id(bout): bout}.values()]
        out = sk.interpolate_motions(b, m, bin_[:, :P], out=bout[:, :P])
        assert out.data_ptr() == bout.data_ptr() and out.stride(0) == 3 * (P + 37)
    out = out.cpu().numpy()
    assert int(sk.debug(E)[1].cpu().numpy().sum()) == 0
    if pad is not None:
        for t, before in pad:
            assert torch.equal(t[:, P:], before), "padding rows were written"
    if variant == "strided":
        assert torch.equal(bin_[:, :P], x), "the input was written"
    for e in range(E):
        assert close(out[e], _ref3(e, P, k), 3e-6, what=f"k_skin E={E} P={P} k={k} {variant}"), e
        assert np.array_equal(out[e].view(np.uint32), alone[e].view(np.uint32)), ("differs from the E = 1 run", e)


@pytest.mark.parametrize("E", [1, 7, 8, 9, 17])
def test_skin_environment_counts(E):
    _check_skin(E, 257, 11)


@pytest.mark.parametrize("P", [1, 255, 256, 257, 1000])
def test_skin_point_counts(P):
    _check_skin(9, P, 11)


@pytest.mark.parametrize("k", [1, 7, 8, 11, 16, 19])
def test_skin_weights_per_point(k):
    _check_skin(9, 257, k)


@pytest.mark.parametrize("variant", ["inplace", "strided", "strided_inplace"])
def test_skin_in_place_and_environment_stride(variant):
    _check_skin(9, 257, 11, variant)


@pytest.mark.parametrize("variant", ["plain", "inplace", "strided", "strided_inplace"])
def test_rotate_quats_environment_stride_and_in_place(variant):
    import torch
    from r2s_hip.skinning import Skinning

    E, P, k = 9, 257, 11
    s = _scene3(); w, wi = _weights3(P, k)
    sk = Skinning(s["rel"], w, wi, device="cuda:0")
    b, m, x, q = _cuda(s["bones"][:E]), _cuda(s["mot"][:E]), _cuda(s["xyz"][:E, :P]), _cuda(s["quat"][:E, :P])
    alone = []
    for e in range(E):   # rotate_quats uses the rotations of the LAST interpolate_motions call
        sk.interpolate_motions(b[e:e + 1], m[e:e + 1], x[e:e + 1])
        alone.append(sk.rotate_quats(q[e:e + 1])[0])
    alone = torch.stack(alone).cpu().numpy()
    sk.interpolate_motions(b, m, x)
    pad = None
    if variant == "plain":
        out = sk.rotate_quats(q)
    elif variant == "inplace":
        buf = q.clone()
        out = sk.rotate_quats(buf, out=buf)
        assert out.data_ptr() == buf.data_ptr()
    else:
        g = torch.Generator().manual_seed(6)
        bin_ = torch.rand(E, P + 37, 4, generator=g).cuda(); bin_[:, :P] = q
        bout = bin_ if variant == "strided_inplace" else torch.rand(E, P + 37, 4, generator=g).cuda()
        pad = [(t, t[:, P:].clone()) for t in {id(bin_): bin_, id(bout): bout}.values()]
        out = sk.rotate_quats(bin_[:, :P], out=bout[:, :P])
        assert out.data_ptr() == bout.data_ptr() and out.stride(0) == 4 * (P + 37)
    out = out.cpu().numpy()
    if pad is not None:
        for t, before in pad:
            assert torch.equal(t[:, P:], before), "padding rows were written"
    for e in range(E):
        assert close(out[e], _refq3(e, P, k), 3e-6, what=f"k_skin_quat {variant}"), e
        assert np.array_equal(out[e].view(np.uint32), alone[e].view(np.uint32)), ("differs from the E = 1 run", e)


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. quaternion branches
# (1,1,1)/sqrt(3) itself ties m00 = m11 = m22 at every angle (and 120 degrees about it has trace 0): a bone may then legitimately take
# another branch.  The diagonal axis is therefore tilted to (1, 0.9, 0.8) and 120 degrees nudged to 121, which keeps every comparison
# of every bone more than 1e-3 from its boundary (asserted below).  60 degrees is there for the trace > 0 branch.
TILT = (1.0, 0.9, 0.8)
ROTATIONS = [(ax, deg) for ax in ((1, 0, 0), (0, 1, 0), (0, 0, 1), TILT) for deg in (170, 179, 180)] + [(TILT, 121), (TILT, 60)]
ROT_IDS = [f"{'xyzd'[((1, 0, 0), (0, 1, 0), (0, 0, 1), TILT).index(ax)]}{deg}" for ax, deg in ROTATIONS]
BRANCH_MARGIN = 1e-3


def quat_branch(R, d=(0.0, 0.0, 0.0, 0.0)):
    """Branch of rotmat_to_quat taken for R with its four comparison quantities moved by d."""
    if R[0, 0] + R[1, 1] + R[2, 2] + d[0] > 0:
        return 0
    if R[0, 0] - R[1, 1] + d[1] > 0 and R[0, 0] - R[2, 2] + d[2] > 0:
        return 1
    return 2 if R[1, 1] - R[2, 2] + d[3] > 0 else 3


def robust_quat_branch(R):
    """The branch, if it is the same however the comparison quantities move by +-BRANCH_MARGIN; else -1."""
    got = {quat_branch(R, (a, b, c, d)) for a in (-BRANCH_MARGIN, BRANCH_MARGIN) for b in (-BRANCH_MARGIN, BRANCH_MARGIN)
           for c in (-BRANCH_MARGIN, BRANCH_MARGIN) for d in (-BRANCH_MARGIN, BRANCH_MARGIN)}
    return got.pop() if len(got) == 1 else -1


@functools.lru_cache(maxsize=None)
def _scene4(i):
    from oracle import lbs_oracle

    s = _scene3()
    bones = s["bones"][0]
    mot = (bones.astype(np.float64) @ (_axis_angle(*ROTATIONS[i]) - np.eye(3)).T).astype(np.float32)
    R, rank = lbs_oracle.bone_rotations(bones, mot, s["rel"])
    assert rank.min() >= 2
    return bones, mot, [robust_quat_branch(r.astype(np.float64)) for r in R]


def test_quaternion_cases_reach_every_branch_with_margin():
    branches = set()
    for i in range(len(ROTATIONS)):
        br = _scene4(i)[2]
        assert min(br) >= 0, (ROT_IDS[i], "a bone is within 1e-3 of a branch boundary")
        branches |= set(br)
    assert branches == {0, 1, 2, 3}


@pytest.mark.parametrize("i", range(len(ROTATIONS)), ids=ROT_IDS)
def test_rotate_quats_large_rotation(i):
    from oracle import lbs_oracle
    from r2s_hip.skinning import Skinning

    P, k = 257, 16
    s = _scene3(); w, wi = _weights3(P, k)
    bones, mot, br = _scene4(i)
    assert min(br) >= 0, "precondition: every bone more than 1e-3 from every branch boundary"
    sk = Skinning(s["rel"], w, wi, device="cuda:0")
    xyz, quat = s["xyz"][0, :P], s["quat"][0, :P]
    out = sk.interpolate_motions(_cuda(bones), _cuda(mot), _cuda(xyz))
    rot = sk.rotate_quats(_cuda(quat))
    assert int(sk.debug(1)[1][0]) == 0
    assert close(out, lbs_oracle.interpolate_motions(bones, mot, s["rel"], xyz, w, wi), 3e-6, what=f"xyz {ROT_IDS[i]}")
    assert close(rot, lbs_oracle.rotate_quats(bones, mot, s["rel"], quat, w, wi), 3e-6, what=f"quat {ROT_IDS[i]}")
