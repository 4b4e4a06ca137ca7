"""pp.nbr_filter, pp.knn_filter and pp.voxel_filter on the device (csrc/cloud_filter.hip) against the tensor formulation on the same
GPU:  python tools/bench_cloud_filter.py [--rounds 3] [--reps 50]

fp32 clouds [N, 4] (three coordinates and an intensity) at N = 2e4, 1e5, 1e6.  Device events round `reps` calls; the two routes
alternate `rounds` times in one process after a warm-up of every shape; the median round is reported.  The tensor route of the two
neighbour filters is run at N = 2e4 only (its [chunk, N, 3] temporaries grow with N^2), that of voxel_filter at all three sizes.  The
radius leaves a few neighbours inside; the voxel size leaves about N / 3 cells (eight points per cell at the centre of the
cloud, fewer in its tails).  For voxel_filter the three stages -- keys (two launches), torch.sort, heads + cumsum + reduce +
stitch -- are also timed on their own, and the sort's share of their sum is reported.  Nothing is asserted; one JSON line per row.

--rows grid runs instead the neighbour filters through the grid index against the brute-force kernels (grid_rows below)."""
import argparse
import json
import math
import statistics
import sys

import torch

sys.path.insert(0, __file__.rsplit("/", 2)[0])
import pypose_amd as pp                                    # noqa: E402
from pypose_amd import _C                                  # noqa: E402
from pypose_amd.function import geometry as geo           # noqa: E402
from tools.bench_knn import alternate, cloud as knn_cloud, timed   # noqa: E402

SIZES = (20_000, 100_000, 1_000_000)
TENSOR_NBR_LIMIT = 20_000


def tensor_route(fn):
    """``fn`` with the kernel route switched off"""
    def run():
        taken = geo._filter_on_kernels
        try:
            geo._filter_on_kernels = lambda *a, **k: False
            return fn()
        finally:
            geo._filter_on_kernels = taken
    return run


def voxel_stages(cloud, voxel):
    """callables for the three stages of geo._voxel_launch on ``cloud``, each on buffers the stage before it has filled"""
    N, D = cloud.shape
    dev, dt = cloud.device, cloud.dtype
    lib, sfx, nwg = _C.library(), _C._SUFFIX[dt], -(-N // 256)
    keys, part = torch.empty(N, dtype=torch.int64, device=dev), torch.empty((256, 3), dtype=dt, device=dev)
    flag, heads = torch.zeros(1, dtype=torch.int32, device=dev), torch.empty(nwg, dtype=torch.int32, device=dev)
    v = [float(torch.tensor(s, dtype=torch.float32)) for s in voxel]
    st = _C.stream_ptr(dev)

    def make_keys():
        _C.check(lib.symbol("pplie_voxel_keys" + sfx, geo._CF_KEYS_SIG)(cloud.data_ptr(), N, D, *v, part.data_ptr(), keys.data_ptr(),
                                                                        flag.data_ptr(), st), "pplie_voxel_keys")
    make_keys()
    skeys, perm = torch.sort(keys, stable=True)
    M = int((skeys[1:] != skeys[:-1]).sum()) + 1
    out = torch.empty((M, D), dtype=dt, device=dev)
    start, count = torch.empty(M, dtype=torch.int32, device=dev), torch.empty(M, dtype=torch.int32, device=dev)
    lead, tail = (torch.empty((nwg, 16), dtype=torch.float64, device=dev) for _ in range(2))
    info = torch.empty((nwg, 4), dtype=torch.int32, device=dev)

    def reduce():
        _C.check(lib.symbol("pplie_voxel_heads", geo._CF_HEADS_SIG)(skeys.data_ptr(), N, heads.data_ptr(), st), "pplie_voxel_heads")
        base = torch.cumsum(heads, dim=0) - heads
        _C.check(lib.symbol("pplie_voxel_reduce" + sfx, geo._CF_REDUCE_SIG)(skeys.data_ptr(), perm.data_ptr(), cloud.data_ptr(),
                                                                            base.data_ptr(), lead.data_ptr(), tail.data_ptr(),
                                                                            info.data_ptr(), out.data_ptr(), start.data_ptr(),
                                                                            count.data_ptr(), N, D, st), "pplie_voxel_reduce")
    return [make_keys, lambda: torch.sort(keys, stable=True), reduce], M


def grid_rows(a, dev, g):
    """--rows grid: the neighbour filters through the grid index (csrc/nbr_grid.hip, csrc/knn_grid.hip) against the brute-force
    kernels of the same build, section 3.9's protocol and clouds: fp32 [N, 4], a radius with about ten neighbours inside, nbr = 5,
    knn_filter at k = 8 with that radius.  Per callable the three rounds are kept (median and spread).  The grid route as the user
    gets it builds its index inside the call; the stages are also timed on an index built before: build, count (with and without
    the early stop), nbr_filter (count + finish + compaction), knn_filter without a radius (list query + finish)."""
    for kind in ("uniform", "surface"):
        for n in SIZES:
            pts = torch.cat([knn_cloud(kind, n, g, dev, torch.float32), torch.rand(n, 1, generator=g, device=dev)], 1)
            xyz = pts[:, :3].contiguous()
            radius = (30 / (4 * math.pi * n)) ** (1 / 3) if kind == "uniform" else (30 / (math.pi * n)) ** 0.5
            r2, index = geo._radius2(radius, pts.dtype), geo.knn_index(xyz)
            fns = {"nbr_brute": lambda: pp.nbr_filter(pts, 5, radius, pdim=3, _grid=False),
                   "nbr_grid": lambda: pp.nbr_filter(pts, 5, radius, pdim=3, _grid=True),
                   "knn_brute": lambda: pp.knn_filter(pts, 8, pdim=3, radius=radius, _grid=False),
                   "knn_grid": lambda: pp.knn_filter(pts, 8, pdim=3, radius=radius, _grid=True),
                   "build": lambda: geo.knn_index(xyz),
                   "count_stop5": lambda: geo._nbr_counts_grid(index, r2, 5, 1, n),
                   "count_exact": lambda: geo._nbr_counts_grid(index, r2, 2 ** 31 - 1, 1, n),
                   "nbr_on_index": lambda: pp.nbr_filter(pts, 5, radius, pdim=3, _grid=index),
                   "query_finish_k8": lambda: pp.knn_filter(pts, 8, pdim=3, _grid=index)}
            for f in fns.values():
                f()
            torch.cuda.synchronize()
            reps = a.reps if n < 1_000_000 else max(2, a.reps // 25)
            times = {name: [] for name in fns}
            for _ in range(a.rounds):
                for name, f in fns.items():
                    times[name].append(timed(f, reps if "brute" in name else a.reps))
            same = (torch.equal(fns["nbr_brute"](), fns["nbr_grid"]()) and torch.equal(fns["knn_brute"](), fns["knn_grid"]()))
            counts = fns["count_exact"]().view(-1)
            print(json.dumps({"op": "nbr_grid", "cloud": kind, "dtype": "torch.float32", "N": n, "D": 4, "radius": radius, "reps_brute": reps, "reps": a.reps,
                              "mean_neighbours": counts.double().mean().item() - 1, "kept": fns["nbr_brute"]().shape[0],
                              "cells": index.cells, "same_results": same,
                              "median_s": {k: statistics.median(v) for k, v in times.items()}, "rounds_s": times}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rows", choices=("filters", "grid"), default="filters")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_cloud_filter needs the GPU"
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    if a.rows == "grid":
        return grid_rows(a, dev, g)
    for n in SIZES:
        cloud = torch.randn(n, 4, generator=g, device=dev)
        radius = 2.5 * n ** (-1 / 3)
        voxel = [6.0 * n ** (-1 / 3)] * 3
        reps = a.reps if n < 1_000_000 else max(2, a.reps // 25)
        fits = n <= TENSOR_NBR_LIMIT
        rows = [("nbr_filter", lambda: pp.nbr_filter(cloud, 2, radius, pdim=3), fits, reps),
                ("knn_filter", lambda: pp.knn_filter(cloud, 8, pdim=3, radius=radius), fits, reps),
                ("voxel_filter", lambda: pp.voxel_filter(cloud, voxel), True, a.reps)]
        for op, fn, with_tensor, r in rows:
            tk, tt = alternate([fn, tensor_route(fn) if with_tensor else None], a.rounds, r)
            row = {"op": op, "dtype": "torch.float32", "N": n, "D": 4, "kernel_s": tk,
                   "tensor_s": tt if with_tensor else "not run: the [chunk, N, 3] temporaries grow with N^2", "rows_out": fn().shape[0]}
            if op != "voxel_filter":
                row["pairs_per_s"] = n * n / tk
            else:
                stages, M = voxel_stages(cloud, voxel)
                ts = alternate(stages, a.rounds, a.reps)
                row.update(cells=M, keys_s=ts[0], sort_s=ts[1], reduce_s=ts[2], sort_share=ts[1] / sum(ts))
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
