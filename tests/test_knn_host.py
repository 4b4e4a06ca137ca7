"""pp.knn (tensor formulation), pp.utils.ReduceToBason and pp.module.ICP on host tensors; Lie ops through the oracle backend."""
import pytest
import torch

import pypose_amd as pp
from pypose_amd.function import geometry as geo
from tests.oracle_backend import oracle_backend

REF = torch.tensor([[9., 2., 2.], [1., 0., 2.], [0., 1., 1.], [5., 0., 1.], [1., 0., 1.], [5., 5., 3.]])
NBR = torch.tensor([[1., 0., 1.], [1., 6., 2.], [5., 1., 0.], [9., 0., 2.]])


def icp_fixture(seed=0):
    """fp64 (source [257, 3], target [1025, 3], R, t, perm): source = T^-1 (target[perm] + 1e-3 randn), T = (R, t) the small
    motion with rotation vector (0.03, -0.02, 0.05) and translation (0.02, -0.01, 0.03)"""
    g = torch.Generator().manual_seed(seed)
    target = torch.randn(1025, 3, generator=g, dtype=torch.float64)
    perm = torch.randperm(1025, generator=g)[:257]
    w = torch.tensor([0.03, -0.02, 0.05], dtype=torch.float64)
    K = torch.zeros(3, 3, dtype=torch.float64)
    K[0, 1], K[0, 2], K[1, 2] = -w[2], w[1], -w[0]
    R = torch.linalg.matrix_exp(K - K.T)
    t = torch.tensor([0.02, -0.01, 0.03], dtype=torch.float64)
    source = (target[perm] + 1e-3 * torch.randn(257, 3, generator=g, dtype=torch.float64) - t) @ R        # rows R^T (x - t)
    return source, target, R, t, perm


@pytest.mark.parametrize("k, values, indices", [
    (1, [[2.], [1.], [1.4142], [1.4142], [0.], [4.2426]], [[3], [0], [0], [2], [0], [1]]),
    (2, [[2., 4.5826], [1., 4.5826], [1.4142, 5.0990], [1.4142, 4.], [0., 4.2426], [4.2426, 5.]],
     [[3, 2], [0, 2], [0, 2], [2, 0], [0, 2], [1, 2]])])
def test_knn_docstring_examples(k, values, indices):
    out = pp.knn(REF, NBR, k=k)
    assert type(out).__name__ == "topk"
    assert (out.values - torch.tensor(values)).abs().max() <= 1e-4
    assert torch.equal(out.indices, torch.tensor(indices))


def test_knn_other_norm_largest_width_and_chunks(monkeypatch):
    g = torch.Generator().manual_seed(0)
    ref, nbr = torch.randn(2, 37, 2, generator=g), torch.randn(41, 2, generator=g)
    want = (ref.unsqueeze(-2) - nbr).abs().sum(-1).topk(5, largest=True)
    monkeypatch.setattr(geo, "_KNN_CHUNK", 2 * 41 * 2 * 8)            # eight reference points per chunk
    got = pp.knn(ref, nbr, k=5, ord=1, largest=True)
    assert torch.equal(got.indices, want.indices) and torch.equal(got.values, want.values)
    with pytest.raises(RuntimeError, match="out of range"):
        pp.knn(ref, nbr, k=42)


@pytest.mark.parametrize("kwargs, losses, steps", [
    (dict(steps=10, tol=1e-2), [1., 0.5, 0.005, 0.001], 3),                       # below tol at the third step
    (dict(steps=4), [1., 0.5, 0.25, 0.125, 0.0625], 4),                           # the step limit
    (dict(steps=20, patience=2, decreasing=0.1), [1., 0.5, 0.49, 0.485, 0.1], 4)])  # two steps in a row under 10 %
def test_reduce_to_bason_stops_where_the_rules_say(kwargs, losses, steps):
    stepper = pp.utils.ReduceToBason(**kwargs)
    it = iter(losses)
    while stepper.continual():
        stepper.step(torch.tensor(next(it)))
    assert stepper.steps == steps
    stepper.reset()
    assert stepper.continual() and stepper.steps == 0


def test_icp_on_the_host_recovers_the_transform():
    source, target, R, t, _ = icp_fixture()
    with oracle_backend():
        T = pp.module.ICP(stepper=pp.utils.ReduceToBason(steps=6, patience=6))(source, target).matrix()
    assert (T[:3, :3] - R).abs().max() <= 1e-3 and (T[:3, 3] - t).abs().max() <= 1e-3
