"""bench.py --dump-outputs (bench.dump_outputs) on CPU tensors: every array get_obs() hands out plus the particle state, float32,
whole when it fits its share of the cap, otherwise the same seeded sample of its elements in every run."""
from types import SimpleNamespace

import numpy as np
import torch

import bench


class _Rollout:
    def __init__(self, E=2, H=12, W=16, N=50):
        g = torch.Generator().manual_seed(3)
        self.device = "cpu"
        self.col = torch.rand(E, 2, 3, H, W, generator=g)
        self.dep = torch.rand(E, 2, 1, H, W, generator=g)
        self.robot = dict(eef_xyz=torch.rand(E, 3, generator=g), eef_quat=torch.rand(E, 4, generator=g), eef_gripper=torch.rand(E, 1, generator=g))
        self.phys = SimpleNamespace(x=torch.rand(E, N, 3, generator=g), v=torch.rand(E, N, 3, generator=g))

    def get_obs(self):
        return dict(image_list=[self.col[:, 0]], depth_list=[self.dep[:, 0]], image_wrist_list=[self.col[:, 1]], depth_wrist_list=[self.dep[:, 1]],
                    robot=self.robot)


def test_dump_writes_every_output_whole_or_as_a_fixed_sample(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_ELEMS", 9 * 700)           # 9 arrays, 700 elements each at most
    ro = _Rollout()
    shapes = bench.dump_outputs(ro, str(tmp_path / "a"))
    names = {"image_0", "depth_0", "image_wrist_0", "depth_wrist_0", "robot_eef_xyz", "robot_eef_quat", "robot_eef_gripper", "particles_x", "particles_v"}
    assert set(shapes) == names
    full = dict(image_0=ro.col[:, 0], depth_0=ro.dep[:, 0], image_wrist_0=ro.col[:, 1], depth_wrist_0=ro.dep[:, 1], particles_x=ro.phys.x,
                particles_v=ro.phys.v, **{f"robot_{k}": t for k, t in ro.robot.items()})
    total = 0
    for n, t in full.items():
        a = np.load(tmp_path / "a" / f"{n}.npy")
        assert a.dtype == np.float32 and shapes[n] == [list(a.shape), list(t.shape)]
        ref = t.numpy()
        if ref.size <= 700:
            assert np.array_equal(a, ref), n
        else:                                                   # image / wrist image (1152), depth (384 whole), x / v (300 whole)
            idx = np.sort(np.random.default_rng(0).choice(ref.size, 700, replace=False))
            assert a.shape == (700,) and np.array_equal(a, ref.reshape(-1)[idx]), n
        total += a.nbytes
    assert total <= bench.DUMP_ELEMS * 4
    bench.dump_outputs(ro, str(tmp_path / "b"))
    for n in names:
        assert np.array_equal(np.load(tmp_path / "a" / f"{n}.npy"), np.load(tmp_path / "b" / f"{n}.npy")), n


def test_dump_cap_is_within_64_mb():
    assert bench.DUMP_ELEMS * 4 <= 64 << 20
