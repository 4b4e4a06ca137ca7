"""pp.knn and one pp.module.ICP iteration on the device (csrc/knn.hip) against the tensor formulation
norm(ref.unsqueeze(-2) - nbr.unsqueeze(-3)).topk on the same GPU:  python tools/bench_knn.py [--rounds 3] [--reps 20]

Device events round `reps` calls; the two routes alternate `rounds` times in one process after a warm-up of every shape; the median
round is reported.  pairs/s is N1 * N2 / time; its share of the VALU issue bound uses the instruction count per pair of the
partial pass's inner loop (ISA of knn_partial_kernel<float, K>: 12 v_sub, 4 v_mul, 8 v_fmac, 2 v_min, 1 v_cmp per four pairs =
6.75) and 256 CUs x 64 lanes per clock x 2.4 GHz = 3.93e13 lane-instructions/s.  Nothing is asserted; one JSON line per row.

--rows grid adds (``all``) or runs alone the rows of the grid index (csrc/knn_grid.hip; pp.knn_index) against the brute-force
kernels under the same protocol, on a uniform and on a surface-like cloud: index build, query at three occupancies, one ICP
iteration."""
import argparse
import json
import statistics
import sys

import torch

sys.path.insert(0, __file__.rsplit("/", 2)[0])
import pypose_amd as pp                                    # noqa: E402
from pypose_amd.function import geometry as geo           # noqa: E402

VALU_PER_PAIR, LANE_RATE = 6.75, 256 * 64 * 2.4e9
TENSOR_LIMIT = 16e9          # bytes of the [N1, N2, 3] temporary the tensor formulation is run with


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e-3 / reps


def alternate(fns, rounds, reps):
    """median seconds per call of each callable (None: not run), the callables taking turns inside every round"""
    for f in fns:
        if f is not None:
            f()
    torch.cuda.synchronize()
    times = [[] for _ in fns]
    for _ in range(rounds):
        for i, f in enumerate(fns):
            if f is not None:
                times[i].append(timed(f, reps))
    return [statistics.median(t) if t else None for t in times]


def tensor_knn(ref, nbr, k):
    return torch.linalg.norm(ref.unsqueeze(-2) - nbr.unsqueeze(-3), dim=-1).topk(k, dim=-1, largest=False)


def icp_forward(source, target, steps, kernels):
    taken = geo._knn_on_kernels
    try:
        if not kernels:
            geo._knn_on_kernels = lambda *a: False
        return pp.module.ICP(stepper=pp.utils.ReduceToBason(steps=steps, patience=steps + 1, tol=0.0))(source, target)
    finally:
        geo._knn_on_kernels = taken


def cloud(kind, n, g, dev, dtype):
    """uniform: the unit cube.  surface: three faces of it, 1e-3 thick -- what a depth image or a lidar sweep of a room gives"""
    pts = torch.rand(n, 3, generator=g, device=dev, dtype=dtype)
    if kind == "surface":
        face = torch.randint(0, 3, (n,), generator=g, device=dev)
        pts[torch.arange(n, device=dev), face] *= 1e-3
    return pts


def grid_rows(a, dev, g):
    """the grid index (csrc/knn_grid.hip) against the brute-force kernels: index build, query (the ordering of the queries
    included, as pp.knn(ref, index) runs it), one ICP iteration; the occupancy sweep at 1e5 x 1e5, k = 1"""
    dtype = torch.float32
    for kind in ("uniform", "surface"):
        base = (geo._GRID_OCCUPANCY,)
        for n1, n2, k, occs in ((100_000, 100_000, 1, (4.0, 8.0, 16.0)), (100_000, 100_000, 8, base), (1_000, 100_000, 1, base),
                                (1_000_000, 1_000_000, 1, base)):
            ref, nbr = cloud(kind, n1, g, dev, dtype), cloud(kind, n2, g, dev, dtype)
            reps = a.reps if n1 * n2 < 1e11 else 1
            index = [geo.knn_index(nbr, _occupancy=o) for o in occs]
            def brute():                                   # (pp.knn's own switch to the grid off)
                taken, geo._GRID_KNN_MIN = geo._GRID_KNN_MIN, None
                try:
                    return pp.knn(ref, nbr, k=k)
                finally:
                    geo._GRID_KNN_MIN = taken
            t = alternate([brute] + [lambda i=i: pp.knn(ref, i, k=k) for i in index]
                          + [lambda i=i: pp.knn(ref, i, k=k, _order=False) for i in index[:1]]
                          + [lambda: geo.knn_index(nbr, _occupancy=occs[0])], a.rounds, reps)
            same = all(torch.equal(pp.knn(ref, i, k=k).indices, brute().indices) for i in index)
            print(json.dumps({"op": "knn_grid", "cloud": kind, "dtype": str(dtype), "N1": n1, "N2": n2, "k": k, "brute_s": t[0],
                              "grid_s": dict(zip(map(str, occs), t[1:1 + len(occs)])), "grid_unordered_s": t[-2], "build_s": t[-1],
                              "cells": [i.cells for i in index], "same_indices": same}), flush=True)
        n1, n2 = 10_000, 100_000
        target = cloud(kind, n2, g, dev, dtype)
        T = pp.se3(torch.tensor([0.02, -0.01, 0.03, 0.03, -0.02, 0.05], device=dev, dtype=dtype)).Exp()
        source = T.Inv().unsqueeze(-2) @ target[torch.randperm(n2, generator=g, device=dev)[:n1]]

        def icp(steps, min_n2):
            taken, geo._GRID_ICP_MIN_N2 = geo._GRID_ICP_MIN_N2, min_n2
            try:
                return icp_forward(source, target, steps, True)
            finally:
                geo._GRID_ICP_MIN_N2 = taken
        t = alternate([lambda: icp(11, None), lambda: icp(1, None), lambda: icp(11, 0), lambda: icp(1, 0)], a.rounds, 3)
        print(json.dumps({"op": "icp_iteration_grid", "cloud": kind, "dtype": str(dtype), "N1": n1, "N2": n2,
                          "brute_s": (t[0] - t[1]) / 10, "grid_s": (t[2] - t[3]) / 10, "grid_first_iteration_s": t[3],
                          "brute_first_iteration_s": t[1]}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rows", choices=("all", "brute", "grid"), default="all")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_knn needs the GPU"
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    if a.rows != "brute":
        grid_rows(a, dev, g)
    for dtype in (torch.float32, torch.float64) if a.rows != "grid" else ():
        size = torch.finfo(dtype).bits // 8
        for n1, n2 in ((100_000, 100_000), (1_000, 100_000)):
            ref, nbr = torch.randn(n1, 3, generator=g, device=dev, dtype=dtype), torch.randn(n2, 3, generator=g, device=dev, dtype=dtype)
            for k in (1, 8):
                fits = n1 * n2 * 3 * size <= TENSOR_LIMIT
                tk, tt = alternate([lambda: pp.knn(ref, nbr, k=k), (lambda: tensor_knn(ref, nbr, k)) if fits else None], a.rounds,
                                   a.reps if n1 * n2 < 1e9 else max(2, a.reps // 4))
                if fits:
                    same = torch.equal(pp.knn(ref, nbr, k=k).indices, tensor_knn(ref, nbr, k).indices)
                rate = n1 * n2 / tk
                print(json.dumps({"op": "knn", "dtype": str(dtype), "N1": n1, "N2": n2, "k": k, "kernel_s": tk, "pairs_per_s": rate,
                                  "share_of_valu_issue_bound": rate * VALU_PER_PAIR / LANE_RATE,
                                  "tensor_s": tt if fits else f"not run: the temporary is {n1 * n2 * 3 * size / 1e9:.0f} GB",
                                  "same_indices": same if fits else None}), flush=True)
        # one ICP iteration = (11-step forward - 1-step forward) / 10, source moved by a small transform
        n1, n2 = 10_000, 100_000
        target = torch.randn(n2, 3, generator=g, device=dev, dtype=dtype)
        T = pp.se3(torch.tensor([0.02, -0.01, 0.03, 0.03, -0.02, 0.05], device=dev, dtype=dtype)).Exp()
        source = T.Inv().unsqueeze(-2) @ target[torch.randperm(n2, generator=g, device=dev)[:n1]]
        t = alternate([lambda: icp_forward(source, target, 11, True), lambda: icp_forward(source, target, 1, True),
                       lambda: icp_forward(source, target, 11, False), lambda: icp_forward(source, target, 1, False)], a.rounds, 3)
        print(json.dumps({"op": "icp_iteration", "dtype": str(dtype), "N1": n1, "N2": n2, "kernel_s": (t[0] - t[1]) / 10,
                          "tensor_s": (t[2] - t[3]) / 10, "pairs_per_s": n1 * n2 * 10 / (t[0] - t[1])}), flush=True)


if __name__ == "__main__":
    main()
