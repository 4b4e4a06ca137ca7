"""pp.module.EPnP on the host: the tensor formulation against the reference's EPnP (CPU, fp64; Lie ops through the oracle backend),
the reference's six-point case, and csrc/pnp_math.h compiled for the host and held to its identities (plain and sanitised)."""
import functools
import os
import subprocess

import pytest
import torch

import pypose_amd as pp
from oracle import ref_loader
from tests.oracle_backend import oracle_backend

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def problems(N, noise, B=64):
    """fp64 (points [B, N, 3], pixels [B, N, 2], K [B, 3, 3], T [B, 7]): focal lengths in [500, 800], principal point (320, 240),
    camera-frame points with z in [4, 8] and x, y within 0.4 z, a random rotation, a translation of 3 randn, points = T^-1 p_cam,
    pixels = the exact projection + noise randn"""
    g = torch.Generator().manual_seed(N)
    rand = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64)
    randn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    K = torch.zeros(B, 3, 3, dtype=torch.float64)
    K[:, 0, 0], K[:, 1, 1], K[:, 0, 2], K[:, 1, 2], K[:, 2, 2] = 500 + 300 * rand(B), 500 + 300 * rand(B), 320, 240, 1
    z = 4 + 4 * rand(B, N, 1)
    cam = torch.cat([(2 * rand(B, N, 2) - 1) * 0.4 * z, z], dim=-1)
    q = randn(B, 4)
    T = torch.cat([3 * randn(B, 3), q / q.norm(dim=-1, keepdim=True)], dim=-1)
    rp = ref_loader.load()
    points = rp.SE3(T).Inv().unsqueeze(-2).Act(cam)
    pixels = rp.point2pixel(cam, K) + noise * randn(B, N, 2)
    return points, pixels, K, T


def pose_distance(est, T):
    """(rotation, translation) parts of |Log(est T^-1)| per problem, in fp64 on the host"""
    rp = ref_loader.load()
    d = (rp.SE3(est.double().cpu()) @ rp.SE3(T).Inv()).Log().tensor()
    return d[..., 3:].norm(dim=-1), d[..., :3].norm(dim=-1)


@pytest.mark.parametrize("noise", [0.0, 0.5])
@pytest.mark.parametrize("refine", [False, True])
@pytest.mark.parametrize("N", [6, 33])
def test_tensor_formulation_matches_the_reference(N, refine, noise):
    """the same algorithm on the same library calls, on the same full batch: rounding only (1e-9 in |Log|)"""
    points, pixels, K, _ = problems(N, noise)
    want = ref_loader.load().module.EPnP(refine=refine)(points, pixels, K).tensor()
    with oracle_backend():
        got = pp.module.EPnP(refine=refine)(points, pixels, K)
    assert isinstance(got, pp.LieTensor) and got.shape == (64, 7)
    rot, tr = pose_distance(got.tensor(), want)
    print(f"N={N} refine={refine} noise={noise}: rot {rot.max():.2e} tr {tr.max():.2e}")
    assert rot.max() <= 1e-9 and tr.max() <= 1e-9


def test_epnp_6pts():
    """the reference's tests/module/test_pnp.py::test_epnp_6pts, to its own tolerance"""
    pose = torch.tensor([0.0000, -8.0000, 0.0000, 0.0000, -0.3827, 0.0000, 0.9239], dtype=torch.float64)
    K = torch.tensor([[2, 0, 4.5], [0, 2, 4.5], [0, 0, 1]], dtype=torch.float64)
    cam = torch.tensor([[2., 0., 2.], [1., 0., 2.], [0., 1., 1.], [0., 0., 1.], [1., 0., 1.], [5., 5., 3.]], dtype=torch.float64)
    with oracle_backend():
        world = pp.SE3(pose).Inv().Act(cam)
        solved = pp.module.EPnP(intrinsics=K)(world, pp.homo2cart(cam @ K.T))
    torch.testing.assert_close(solved.tensor(), pose, rtol=1e-4, atol=1e-4)


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "sanitised"])
def test_device_math_identities_on_the_host(flags, tmp_path):
    """tests/hostmath/pnp_check.cpp: a stand-alone program around csrc/pnp_math.h; its exit status says whether every identity held"""
    exe = str(tmp_path / "pnp_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", *flags, "-I" + os.path.join(ROOT, "pypose_amd", "csrc"),
                    os.path.join(ROOT, "tests", "hostmath", "pnp_check.cpp"), "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    print(run.stdout, run.stderr)
    assert run.returncode == 0
