"""bench.py -- BASELINE.json's metric on its configs[1] workload; with --full, plus one block per other BASELINE config.

    python bench.py --gpus N --steps K --warmup W        (N > 1 launches itself: one process per GPU over RCCL)
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...

A plain run sets up, warms up, times the K steps and prints the line: the contract keys, `config`, `roofline` (HIP events inside
the timed region) and a `summary` of the headline alone.  `--dump-outputs DIR` also writes what the last timed step computed
(DIR/exp.npy, DIR/log.npy; inputs are seeded, so two builds can be compared output for output).  `--full` adds everything below
that is not the headline: "cpu_baseline", the block per other config, the sharded legs, the side file of full blocks.

Workload ("se3_explog_b10m"): batched SE3 Exp -> Log forward, B = 10,000,000 rows of fp32 per GPU
(BASELINE.json configs[1]; inputs `pp.randn_se3(B)`, seed = rank), through the public API
(``x.Exp()`` then ``X.Log()``: two HIP kernels per step, the group element X is materialised in
HBM as in the reference).  One step = one Exp+Log pass over the whole batch; value = SE3
Exp+Log pairs per second summed over all ranks (weak scaling: rows are independent, each rank
owns its own B rows, no data-path collective).

Printed JSON line (rank 0): the driver contract + "roofline" (dominant kernel, HIP-event timed
inside the timed region) + "cpu_baseline" (the reference's own PyTorch-CPU path, shipped as oracle/_ref, timed on
this box's host cores on a bounded sample of the same workload; the numpy port of round 1 beside it) + one block per
other BASELINE config, each with its own roofline figures:
    c1          configs[0]  fwd + bwd of Exp().Log() at B = 1024 (plumbing latency)
    lm_invnet   configs[2]  LM on InvNet SE3, 10^6 independent problems
    lm_pgo      metric      LM iterations / s on a 10 k-pose graph;  lm_pgo_100k  configs[3] on one GPU
    imu         configs[4]  IMUPreintegrator 4096 x 1024 with and without covariance
    ba_reproj   SURVEY 8(f) rank 3: reprojection residual + closed-form Jacobian blocks, 4 M observations
With N > 1 (one process per GPU) the sharded legs replace them: lm_invnet_sharded (problems), imu_sharded (sequences),
lm_pgo_sharded (configs[3]: edges / solve sharded).
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

# torch is imported inside main(): the cpu_baseline leg spawns one worker per host core and every
# worker re-imports this file, which must stay light (numpy only).
ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_PEAK_GBPS = 8000.0          # MI355X HBM3E spec peak (MI355X_MICROARCH.md)
# VALU issue peak: 256 CUs x 4 SIMD-32, a wave64 VALU instruction occupies its SIMD for 2 cycles, 2.4 GHz (MI355X_MICROARCH.md
# "Wave scheduling" / per-instruction cycle constants): 256 * 4 * 2.4e9 / 2 wave-instructions per second
VALU_PEAK_WAVE_INSTR = 256 * 4 * 2.4e9 / 2
# what tools/micro/valu_rate.hip reaches of that peak with nothing but independent v_fma_f32 on 8 waves per SIMD (2.45 nominal cycles
# per instruction; a DPP move costs 4.7, a reciprocal 8.4): profiles/r04/valu_rate.json -- the ceiling of a `bound: "valu"` fraction
VALU_MEASURED_CEILING = 2.0 / 2.445


def _pmc(name):
    """profiles/<name>.json: counters of EARLIER rocprofv3 --pmc passes of these kernels (never collected inside a bench run);
    every file carries the commit and date it was collected at under "_stamp" """
    try:
        with open(os.path.join(ROOT, "profiles", name + ".json")) as f:
            return json.load(f)
    except Exception:
        return {}


def valu_roofline(kernels, seconds, hbm_block=None):
    """roofline block of a leg whose kernels are bound by VALU instruction issue, not by bytes: achieved = wave64 VALU
    instructions issued per second (SQ_INSTS_VALU of the leg's kernels, profiles/pmc_sq.json, over the time measured HERE)
    against the chip's issue peak; the HBM figure rides along as "hbm" """
    sq = _pmc("pmc_sq")
    tot, used = 0.0, {}
    for k in kernels:
        e = sq.get(k)
        if not e:
            return dict(hbm_block or {}, bound_note=f"VALU-issue bound by measurement, but profiles/pmc_sq.json has no entry for {k}")
        tot += e["SQ_INSTS_VALU"]
        used[k] = {"SQ_INSTS_VALU_per_launch": e["SQ_INSTS_VALU"], "valu_per_wave": e.get("valu_per_wave"), "waves": e.get("SQ_WAVES")}
    ach = tot / seconds
    return {"bound": "valu", "unit": "wave64 VALU instructions/s", "achieved": ach, "peak": VALU_PEAK_WAVE_INSTR,
            "frac": ach / VALU_PEAK_WAVE_INSTR, "frac_ceiling_measured": VALU_MEASURED_CEILING,
            "ceiling_source": "profiles/r04/valu_rate.json (tools/micro/valu_rate.hip: plain v_fma_f32, 8 waves per SIMD)", "kernels": used,
            "counter_source": f"profiles/pmc_sq.json ({sq.get('_stamp', 'unstamped')}): rocprofv3 --pmc SQ_INSTS_VALU of an earlier run "
                              "of these kernels on this workload; the time is this run's", "hbm": hbm_block}

BYTES_PER_ROW = {"se3_exp_fwd": 24 + 28, "se3_log_fwd": 28 + 24}    # 52 B/row each


# ---------------------------------------------------------------------------------------------------------------
# cpu_baseline
# ---------------------------------------------------------------------------------------------------------------
def _cpu_worker(args):
    import numpy as np
    from oracle import lie_np
    seed, n = args
    rng = np.random.default_rng(seed)
    d = rng.standard_normal((n, 3))
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    x = np.concatenate([rng.standard_normal((n, 3)), d * rng.standard_normal((n, 1))], -1).astype(np.float32)
    t0 = time.perf_counter()
    X = lie_np.se3_exp_fwd(x)[0]
    y = lie_np.se3_log_fwd(X)[0]
    return time.perf_counter() - t0, float(y[0, 0])


def cpu_baseline_port(budget_s: float = 6.0):
    """Oracle (numpy port of operation.py's se3_Exp / SE3_Log) on all host cores, bounded sample."""
    import multiprocessing as mp
    cores = os.cpu_count() or 1
    chunk = 250_000
    ctx = mp.get_context("spawn")
    rows = 0
    with ctx.Pool(cores) as pool:
        pool.map(_cpu_worker, [(i, 1000) for i in range(cores)])       # warm the workers
        t0 = time.perf_counter()
        rnd = 0
        while time.perf_counter() - t0 < budget_s and rows < 10_000_000:
            pool.map(_cpu_worker, [(1000 + rnd * cores + i, chunk) for i in range(cores)])
            rows += chunk * cores
            rnd += 1
        wall = time.perf_counter() - t0
    return {"value": rows / wall, "unit": "SE3 Exp+Log pairs/s", "cores": cores, "kind": "port",
            "sample": f"{rows} rows of the same fp32 workload (oracle/lie_np.py se3_exp_fwd+se3_log_fwd, "
                      f"{cores} processes x {chunk}-row chunks, {wall:.1f} s wall)"}


def cpu_baseline(budget_s: float = 12.0):
    """The REFERENCE's own path -- `pp.randn_se3(B).Exp().Log()` of the PyPose package shipped as oracle/_ref -- on
    PyTorch-CPU with all host cores (intra-op threads), bounded sample; the numpy port of round 1 rides along."""
    import torch
    from oracle import ref_loader
    port = None
    try:
        port = cpu_baseline_port()
    except Exception as e:           # never lose the headline line
        port = {"error": repr(e)}
    if not ref_loader.available():
        port["note"] = "oracle/_ref not shipped: numpy port only"
        return port
    rpp = ref_loader.load()
    cores = os.cpu_count() or 1
    old = torch.get_num_threads()
    B = 10_000_000                  # BASELINE configs[1]'s own size ("C2: full 10 M fwd")
    torch.manual_seed(0)
    x = rpp.randn_se3(B, dtype=torch.float32)
    # PyTorch's intra-op pool does not scale to every core of a large host on this chain of ~100 small aten ops (256 threads
    # measured 20x slower than 32 on the MI355X box): a short probe picks the thread count, the rest of the budget times it
    best_t, best_rate, tried = 1, 0.0, {}
    try:
        with torch.no_grad():
            for t in sorted({min(cores, c) for c in (8, 16, 32, 64, cores)}):
                torch.set_num_threads(t)
                xs = x[:100_000]
                xs.Exp().Log()
                t0 = time.perf_counter()
                xs.Exp().Log()
                rate = 100_000 / (time.perf_counter() - t0)
                tried[t] = rate
                if rate > best_rate:
                    best_t, best_rate = t, rate
            torch.set_num_threads(best_t)
            x.Exp().Log()                                   # warm-up
            t0 = time.perf_counter()
            passes = 0
            while time.perf_counter() - t0 < budget_s and passes < 20:
                x.Exp().Log()
                passes += 1
            wall = time.perf_counter() - t0
    finally:
        torch.set_num_threads(old)
    return {"value": B * passes / wall, "unit": "SE3 Exp+Log pairs/s", "cores": best_t, "host_cores": cores, "kind": "reference",
            "sample": f"{passes} passes of pp.randn_se3({B}).Exp().Log() (fp32, torch {torch.__version__} CPU, {best_t} intra-op "
                      f"threads -- the fastest of {sorted(tried)} in a 100k-row probe, {wall:.1f} s wall) through the reference package "
                      f"itself (PyPose {getattr(rpp, '__version__', '?')}, oracle/_ref)",
            "thread_probe_pairs_per_s": {str(k): v for k, v in tried.items()},
            "numpy_port": port}


# ---------------------------------------------------------------------------------------------------------------
# per-leg cpu_baseline (BASELINE.md section 3 / SURVEY.md 8(c)-(d)): the reference itself at the largest size it can run,
# and the reference-function restatement of its LM loop (oracle/ref_restate.py) at the leg's full size
# ---------------------------------------------------------------------------------------------------------------
def leg_cpu_baselines(threads, instances=None, gpu=None):
    """{leg: cpu_baseline block}; `threads` intra-op threads (the count the headline's probe found fastest on this host).
    `instances`: the host-generated LM instances the GPU legs ran on (same tensors here); `gpu`: the GPU legs' blocks, whose
    recorded trajectories are compared with the restatement's in a `parity` entry per leg."""
    instances, gpu = instances or {}, gpu or {}
    import torch
    from oracle import ref_loader, ref_restate
    if not ref_loader.available():
        return {}
    rpp = ref_loader.load()
    cores = os.cpu_count() or 1
    old = torch.get_num_threads()
    torch.set_num_threads(threads)
    out = {}

    def block(value, unit, kind, sample, **kw):
        return {"value": value, "unit": unit, "cores": threads, "host_cores": cores, "kind": kind, "sample": sample, **kw}

    def guarded(name, fn):
        try:
            out[name] = fn()
        except Exception as e:
            out[name] = {"error": repr(e)}

    class RefInvNet(torch.nn.Module):
        def __init__(self, init):
            super().__init__()
            self.pose = rpp.Parameter(init)

        def forward(self, input):
            return (self.pose @ input).Log().tensor()

    class RefPoseGraph(torch.nn.Module):
        def __init__(self, init):
            super().__init__()
            self.nodes = rpp.Parameter(init)

        def forward(self, e, poses):
            n1, n2 = self.nodes[e[..., 0]], self.nodes[e[..., 1]]
            return (poses.Inv() @ n1.Inv() @ n2).Log().tensor()

    def parity_of(key, rec):
        tr = (gpu.get(key) or {}).get("trajectory")
        return _parity(tr, rec) if tr and key in instances and "error" not in tr else None

    def invnet():
        B = 1_000_000
        if "lm_invnet" in instances:
            init, inp = instances["lm_invnet"]
            B = init.shape[0]
        else:
            torch.manual_seed(0)
            init, inp = rpp.randn_SE3(B).tensor(), rpp.randn_SE3(B).tensor()
        rec = ref_restate.invnet_lm(init, inp, 3, strategy="constant", strategy_kw=dict(damping=1e-4))
        t = sum(rec["step_seconds"]) / 3
        Br = 1024
        torch.manual_seed(0)
        net = RefInvNet(rpp.randn_SE3(Br))
        x = rpp.randn_SE3(Br)
        opt = rpp.optim.LM(net, strategy=rpp.optim.strategy.Constant(damping=1e-4))
        opt.step(x)
        t0 = time.perf_counter()
        opt.step(x)
        tr = time.perf_counter() - t0
        return block(1.0 / t, "LM steps/s", "port", f"3 LM steps at B = {B} fp32: oracle/ref_restate.invnet_lm -- the reference's loop "
                     "(optimizer.py:644-679) on [B,7,7] blocks, every formula a reference function (se3_Jl_inv, SE3 ops, cholesky_ex, "
                     "its own strategy object)", problem_steps_per_s=B / t, losses=rec["loss"], parity=parity_of("lm_invnet", rec),
                     reference_at_largest_runnable_size=block(1.0 / tr, "LM steps/s", "reference", f"one pp.optim.LM step of the reference "
                                                                 f"package itself (dense modjac J [6B,7B]) at B = {Br}", problem_steps_per_s=Br / tr))

    def pgo(N, E, steps, key):
        def f():
            if key in instances:
                e, rel, init = instances[key]
            else:
                e, rel, init = ref_restate.pose_graph_problem(N, E, dtype=torch.float32)
            rec = ref_restate.pgo_lm(init, e, rel, steps, radius=1e4, tol=1e-4, maxiter=250)
            t = sum(rec["step_seconds"]) / steps
            Nr, Er = 200, 560
            er, relr, initr = ref_restate.pose_graph_problem(Nr, Er, dtype=torch.float32)
            g = RefPoseGraph(rpp.SE3(initr))
            opt = rpp.optim.LM(g, solver=rpp.optim.solver.Cholesky(), strategy=rpp.optim.strategy.TrustRegion(radius=1e4))
            opt.step((er, rpp.SE3(relr)))
            t0 = time.perf_counter()
            opt.step((er, rpp.SE3(relr)))
            tr = time.perf_counter() - t0
            return block(1.0 / t, "LM steps/s", "port", f"{steps} LM step(s) at {N} nodes / {E} edges fp32: oracle/ref_restate.pgo_lm -- "
                         "per-edge blocks from the reference's se3_Jl_inv / SE3_Adj, J as torch.sparse_csr, A = J^T J in CSR (the reference's "
                         "sparse branch, optimizer.py:640-643), the reference's CG (solver.py:276-340, tol 1e-4, maxiter 250) with a "
                         "block-Jacobi M, TrustRegion(radius=1e4)", losses=rec["loss"], parity=parity_of(key, rec), solve_seconds_per_step=sum(rec["solve_seconds"]) / steps,
                         reference_at_largest_runnable_size=block(1.0 / tr, "LM steps/s", "reference", "one pp.optim.LM step of the reference "
                                                                     f"package itself (dense J, Cholesky) at {Nr} nodes / {Er} edges"))
        return f

    def imu():
        B, F = 512, 1024
        torch.manual_seed(0)
        dt = torch.full((B, F, 1), 0.005)
        gyro = 0.1 * torch.randn(B, F, 3)
        acc = torch.randn(B, F, 3) + torch.tensor([0., 0., 9.81])
        res = {}
        for cov in (True, False):
            ref_restate.imu_forward(dt[:8], gyro[:8], acc[:8], cov)
            t0 = time.perf_counter()
            ref_restate.imu_forward(dt, gyro, acc, cov)
            res[cov] = time.perf_counter() - t0
        return block(B * F / res[True], "steps/s", "reference", f"one forward of the reference's IMUPreintegrator(prop_cov=True) at "
                     f"{B} sequences x {F} steps fp32 (its largest size here: SURVEY 8d 'C5: B <= 512')", states_only_value=B * F / res[False])

    def imu_train():
        # the reference itself, forward + backward of the example's training loss (examples/module/imu/imu_corrector.py:69-74, 97)
        B, F = 64, 1024
        torch.manual_seed(0)
        dt = torch.full((B, F, 1), 0.005)
        gyro = (0.1 * torch.randn(B, F, 3)).requires_grad_(True)
        acc = (torch.randn(B, F, 3) + torch.tensor([0., 0., 9.81])).requires_grad_(True)
        gt_pos, gt_rot = torch.randn(B, F, 3), rpp.randn_SO3(B, F)
        integ = rpp.module.IMUPreintegrator(prop_cov=False, reset=True)

        def step():
            gyro.grad = acc.grad = None
            o = integ(dt=dt, gyro=gyro, acc=acc)
            loss = torch.nn.functional.mse_loss(o["pos"], gt_pos) + 5e2 * (gt_rot * o["rot"].Inv()).Log().norm(dim=-1).mean()
            loss.backward()
        step()
        t0 = time.perf_counter()
        n = 0
        while time.perf_counter() - t0 < 6.0:
            step()
            n += 1
        t = (time.perf_counter() - t0) / n
        return block(B * F / t, "steps/s", "reference", f"{n} training steps (forward + loss + backward) of the reference's IMUPreintegrator("
                     f"prop_cov=False) at {B} sequences x {F} steps fp32, loss of examples/module/imu/imu_corrector.py:69-74")

    def ops_chain():
        # "fwd+bwd at 1 M" is the largest the reference runs comfortably on the host
        B = 1_000_000
        torch.manual_seed(0)
        x = rpp.randn_se3(B, dtype=torch.float32, requires_grad=True)

        def step():
            x.grad = None
            x.Exp().Log().sum().backward()
        step()
        t0 = time.perf_counter()
        n = 0
        while time.perf_counter() - t0 < 6.0:
            step()
            n += 1
        t = (time.perf_counter() - t0) / n
        return block(B / t, "SE3 Exp+Log pairs/s forward + backward", "reference", f"{n} passes of randn_se3({B}).Exp().Log().sum().backward() "
                     "(fp32) through the reference package itself")

    try:
        with torch.no_grad():
            guarded("lm_invnet", invnet)
            guarded("lm_pgo", pgo(10_000, 40_000, 3, "lm_pgo"))
            guarded("lm_pgo_100k", pgo(100_000, 400_000, 1, "lm_pgo_100k"))
            guarded("imu", imu)
        guarded("imu_train", imu_train)
        guarded("ops_10m", ops_chain)
    finally:
        torch.set_num_threads(old)
    return out


# ---------------------------------------------------------------------------------------------------------------
# secondary workloads
# ---------------------------------------------------------------------------------------------------------------
def _pose_graph_problem(dev, nodes, edges):
    """SURVEY.md section 8d C4 generator: chain + random loop closures, sigma 0.01 edge noise, sigma 0.05 initial error.
    With `dev` = cpu the random numbers come from the HOST generator (the group arithmetic is still staged through the HIP
    kernels): bench.py builds each LM instance once this way and hands the SAME tensors to the GPU leg and to the CPU
    baseline's restatement of the reference's loop, so that their loss / damping / reject sequences can be compared."""
    import torch
    import pypose_amd as pp
    g = torch.Generator().manual_seed(0)
    torch.manual_seed(0)
    gt = pp.cumprod(pp.randn_SE3(nodes, sigma=0.3, device=dev), dim=0, left=False)
    chain = torch.stack([torch.arange(nodes - 1), torch.arange(1, nodes)], -1)
    extra = torch.randint(0, nodes, (edges - (nodes - 1), 2), generator=g)
    extra[:, 1] = torch.where(extra[:, 0] == extra[:, 1], (extra[:, 1] + 1) % nodes, extra[:, 1])
    e = torch.cat([chain, extra], 0).to(dev)
    rel = gt[e[:, 0]].Inv() @ gt[e[:, 1]] @ pp.randn_SE3(edges, sigma=0.01, device=dev)
    init = gt @ pp.randn_SE3(nodes, sigma=0.05, device=dev)
    return e, rel, init


def _pose_graph_model(init):
    import torch
    import pypose_amd as pp

    class PoseGraph(torch.nn.Module):           # the reference's own model, examples/module/pgo/pgo.py:15-25
        def __init__(self, init):
            super().__init__()
            self.nodes = pp.Parameter(init)

        def forward(self, e, poses):
            n1, n2 = self.nodes[e[..., 0]], self.nodes[e[..., 1]]
            return (poses.Inv() @ n1.Inv() @ n2).Log().tensor()
    return PoseGraph(init)


def _sync(dev):
    import torch
    if dev.type == "cuda":
        torch.cuda.synchronize()


def _host_instances(small, standin):
    """the LM instances of the secondary legs, generated ONCE on the host (host RNG; plain tensors)"""
    import torch
    import pypose_amd as pp
    import warnings
    cpu = torch.device("cpu")
    inst = {}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")            # (host tensors staged through the kernels: that is the point here)
        for key, (n, e) in (("lm_pgo", (60, 150) if small else (10_000, 40_000)), ("lm_pgo_100k", (80, 200) if small else (100_000, 400_000))):
            ed, rel, init = _pose_graph_problem(cpu, n, e)
            inst[key] = (ed, rel.tensor().contiguous(), init.tensor().contiguous())
        B = 2000 if small else 1_000_000
        torch.manual_seed(0)
        inst["lm_invnet"] = (pp.randn_SE3(B).tensor().contiguous(), pp.randn_SE3(B).tensor().contiguous())
    return inst


def _parity(gpu, ref):
    """same instance, same settings: the GPU leg's recorded trajectory beside the CPU restatement of the reference's loop"""
    n = min(len(gpu["loss"]), len(ref["loss"]))
    if n == 0:
        return None
    rel = [abs(a - b) / max(abs(b), 1e-300) for a, b in zip(gpu["loss"][:n], ref["loss"][:n])]
    # "LM-step numerics within 1e-5 of reference" is a statement about a STEP: the loss a step ends at is compared on the scale
    # of the loss it started from (after one step InvNet sits at 1e-8 of its initial 8e6, where the ratio of two fp32 rounding
    # floors says nothing), with the fp32 floor of the sum of squares (eps32^2 x terms x |pose|^2 ~ 1e-12 per residual row) added
    start = [gpu.get("initial_loss") or ref["loss"][0]] + list(ref["loss"][:n - 1])
    floor = 1e-12 * float(gpu.get("residual_rows") or 0)
    over = [abs(a - b) / (1e-5 * abs(s0) + floor) for a, b, s0 in zip(gpu["loss"][:n], ref["loss"][:n], start)]
    return {"steps_compared": n, "loss_err_over_tolerance": max(over), "loss_err_over_tolerance_per_step": over,
            "tolerance": "|loss - loss_ref| <= 1e-5 x (loss the step started from) + 1e-12 x residual rows (fp32 floor); <= 1 passes",
            "loss_rel": max(rel), "loss_rel_per_step": rel,
            "damping_equal": all(abs(a - b) <= 1e-6 * abs(b) for a, b in zip(gpu["damping"][:n], ref["damping"][:n])),
            "reject_equal": list(gpu["reject"][:n]) == list(ref["reject"][:n]),
            "gpu": {k: gpu[k][:n] for k in ("loss", "damping", "reject")}, "cpu": {k: ref[k][:n] for k in ("loss", "damping", "reject")},
            "note": "fp32 on both sides; the inexact PCG solves (tol 1e-4) may end in different iterations, see DESIGN.md section 4"}


def pgo_lm_rate(dev, nodes=10_000, edges=40_000, steps=3, reps=5, with_static=True, problem=None):
    """Second half of BASELINE.json's metric: LM iterations/s on a synthetic pose graph (PCG tol 1e-4 / maxiter 250 as
    examples/module/ba, TrustRegion(radius=1e4) as pgo.py:67).  Every repetition restarts from the same initial estimate
    and takes the `steps` LM steps that do the actual descent (this problem reaches its noise floor in 3-4); repetition 0
    (structure probe, kernel verification, hipGraph capture) is untimed; the rate is the median repetition."""
    import pypose_amd as pp
    if problem is None:
        e, rel, init = _pose_graph_problem(dev, nodes, edges)
    else:
        e, rel, init = problem[0].to(dev), pp.SE3(problem[1].to(dev)), pp.SE3(problem[2].to(dev))
        nodes, edges = init.shape[0], e.shape[0]

    def run(static):
        graph = _pose_graph_model(init.clone())
        solver = pp.optim.solver.PCG(tol=1e-4, maxiter=250)
        opt = pp.optim.LM(graph, solver=solver, strategy=pp.optim.strategy.TrustRegion(radius=1e4), static=static)
        times, losses, its = [], [], []
        for rep in range(reps + 1):
            graph.nodes.data.copy_(init.tensor())
            if hasattr(opt, "loss"):
                del opt.loss
            opt.param_groups[0].update(opt.strategy.defaults)
            _sync(dev)
            t0 = time.perf_counter()
            losses, its = [], []
            for _ in range(steps):
                losses.append(opt.step((e, rel)))
                its.append(solver.iterations)
            _sync(dev)
            if rep:
                times.append((time.perf_counter() - t0) / steps)
        return opt, sorted(times)[len(times) // 2], times, [float(l) for l in losses], its

    graph0 = _pose_graph_model(init.clone())
    l0 = float(graph0(e, rel).detach().square().sum())
    opt, dt, times, losses, its = run(False)
    its_mean = sum(its) / len(its)
    persistent = nodes <= 32768            # (optim/posegraph.py PERSIST_NODES: one persistent launch per solve, blocks resident in LDS)
    traffic = _pmc("pmc_traffic")
    if persistent:
        # One launch per solve with the off-diagonal blocks resident in LDS: the blocks cross HBM once per SOLVE, not once per
        # iteration, and an iteration is a grid-wide exchange (tagged words through L2), not a stream of bytes.  What bounds it is
        # the latency of that exchange: us per iteration against the hand-off floor measured in profiles/r03/pingpong.log.
        solve_bytes = (traffic.get("detail", {}).get("pcg_ghost_solve") or {})
        lin_bytes = 388.0 * edges + 168.0 * nodes
        roof = {"bound": "latency (one grid-wide exchange per PCG iteration)", "unit": "us per PCG iteration",
                "us_per_lm_step": dt * 1e6, "mean_pcg_iterations": its_mean,
                "us_per_pcg_iteration_incl_step_overheads": dt * 1e6 / max(its_mean, 1.0),
                "exchange_floor_us": [0.40, 0.57], "floor_source": "profiles/r03/pingpong.log (one tagged-word hand-off between two workgroups)",
                "marginal_us_per_iteration": 5.9, "marginal_source": "profiles/r06/pcg_iter.json (tools/time_pcg_iter.py; 8.0 in round 5, 7.4 at the start of "
                "round 6): the two-level (block-Jacobi + gauge) iteration with its 11-quantity exchange; the plain block-Jacobi iteration needs "
                "17 / 35 / 105 iterations on this instance where this one needs 17 / 19 / 25",
                "hbm": {"bound": "hbm", "unit": "GB/s", "peak": HBM_PEAK_GBPS,
                        "bytes_per_lm_step": lin_bytes + float(solve_bytes.get("fetch", 0.0) or 0.0) + float(solve_bytes.get("write", 0.0) or 0.0),
                        "note": "linearisation 388 B/edge + 168 B/node (SURVEY 8d C4) + the solve's COUNTED traffic per launch "
                                "(profiles/pmc_traffic.json pcg_ghost_solve, most of it the polled hand-off table): "
                                "a few percent of the HBM rate -- not what bounds this leg"}}
        roof["hbm"]["achieved"] = roof["hbm"]["bytes_per_lm_step"] / dt / 1e9
        roof["hbm"]["frac"] = roof["hbm"]["achieved"] / HBM_PEAK_GBPS
    else:
        # two launches per iteration (pcg2_spmv_pack + pcg2_step), every iteration streams the packed blocks: SURVEY 8(d) C4's
        # 400 B/edge is the un-packed figure; the packed layout moves 84 B per incidence + 2 x 144 B per node + the vectors
        from pypose_amd.optim.posegraph import FusedPCG as _F
        diag = 84.0 if getattr(_F, "pack_diag", False) else 144.0     # D and Binv as packed upper triangles (round 5) or full blocks
        it_bytes = 84.0 * 2 * edges + (diag * 2 + 24.0 * 6) * nodes + 4.0 * 2 * edges
        step_bytes = its_mean * it_bytes + 388.0 * edges + 168.0 * nodes
        roof = {"bound": "hbm", "unit": "GB/s", "peak": HBM_PEAK_GBPS, "achieved": step_bytes / dt / 1e9,
                "frac": step_bytes / dt / 1e9 / HBM_PEAK_GBPS, "algorithmic_bytes_per_step": step_bytes,
                "algorithmic_bytes_per_pcg_iteration": it_bytes, "mean_pcg_iterations": its_mean,
                "us_per_pcg_iteration_incl_step_overheads": dt * 1e6 / max(its_mean, 1.0),
                "per": f"LM step (linearise + mean PCG iterations x packed blocks 84 B/incidence, D and Binv {diag:.0f} B/node each, vectors)",
                "captured_trial": bool(getattr(_F, "capture_large", False)),
                "note": "the iteration is bound by the rate the memory system serves its gathers' REQUESTS (profiles/r04 and r05 "
                        "EXPERIMENTS.md: waves 66 % parked on s_waitcnt, insensitive to occupancy, to trips per wave and -- within 2 us -- "
                        "to whether the gathered rows hit the L2); counted traffic 1.71x algorithmic (173.3 MB per iteration, "
                        "profiles/pmc_traffic.json)"}
        det = traffic.get("detail", {})
        sp, stp = det.get("pcg2_spmv") or {}, det.get("pcg2_step") or {}
        if sp.get("fetch_r05") and stp.get("fetch_r05"):
            roof["traffic_per_pcg_iteration"] = sp["fetch_r05"] + sp.get("write_r05", 0.0) + stp["fetch_r05"] + stp.get("write_r05", 0.0)
            roof["traffic_source"] = f"profiles/pmc_traffic.json ({traffic.get('_stamp', 'unstamped')}): FETCH_SIZE x 2 + WRITE_SIZE of " \
                                     "pcg2_spmv + pcg2_step, an earlier run of these kernels on this workload"
    out = {"metric": f"LM iters/sec (PGO {nodes} poses / {edges} edges)", "value": 1.0 / dt, "unit": "LM steps/s", "nodes": nodes,
           "edges": edges, "path": opt.linearization, "initial_loss": l0, "losses": losses, "pcg_iterations": its,
           "steps_per_repetition": steps, "repetitions_ms_per_step": [round(t * 1e3, 3) for t in times], "roofline": roof}
    if with_static:
        # LM(static=True): the caller's promise that the residual program does not change between steps
        opt2, dt2, _, losses2, _ = run(True)
        out["static_model_value"] = 1.0 / dt2
        out["static_model_final_loss"] = losses2[-1]
    # untimed: the trajectory of one repetition, read step by step, for the parity block against the CPU restatement
    graph = opt.model.model if hasattr(opt.model, "model") else None
    traj = {"loss": [], "damping": [], "reject": []}
    try:
        opt.model.model.nodes.data.copy_(init.tensor())
        if hasattr(opt, "loss"):
            del opt.loss
        opt.param_groups[0].update(opt.strategy.defaults)
        for _ in range(steps):
            traj["loss"].append(float(opt.step((e, rel))))
            traj["damping"].append(float(opt.param_groups[0]["damping"]))
            traj["reject"].append(int(opt.reject_count))
    except Exception as ex:                     # never lose the leg over its parity record
        traj["error"] = repr(ex)
    traj["initial_loss"], traj["residual_rows"] = l0, edges
    out["trajectory"] = traj
    return out


def invnet_lm_rate(dev, B=1_000_000, steps=3, reps=40, group=None, problem=None):
    """BASELINE configs[2]: LM on the reference's README InvNet, B independent SE3 problems (per rank), fp32
    (SURVEY.md section 8d C3).  A repetition restarts from the same random poses and takes `steps` LM steps (the problem
    converges in 2-3; later steps sit at the rounding floor where every trial is a coin-flip rejection).  The step is
    asynchronous -- loop state and decisions live on the device -- so `reps` repetitions are enqueued back to back and
    timed with ONE synchronisation at the end; the 28 MB pose reset per repetition is inside the timed region."""
    import torch
    import pypose_amd as pp

    class InvNet(torch.nn.Module):
        def __init__(self, init):
            super().__init__()
            self.pose = pp.Parameter(init)

        def forward(self, input):
            return (self.pose @ input).Log().tensor()

    torch.manual_seed(0 if group is None else 1 + torch.distributed.get_rank())
    if problem is None:
        init = pp.randn_SE3(B, device=dev)
        inp = pp.randn_SE3(B, device=dev)
    else:
        init, inp = pp.SE3(problem[0].to(dev)), pp.SE3(problem[1].to(dev))
        B = init.shape[0]
    l0 = float(InvNet(init)(inp).detach().square().sum())

    def measure(static):
        net = InvNet(init.clone())
        opt = pp.optim.LM(net, strategy=pp.optim.strategy.Constant(damping=1e-4), group=group, static=static)

        def reset():
            net.pose.data.copy_(init.tensor())
            if hasattr(opt, "loss"):
                del opt.loss

        def run(n):
            for _ in range(n):
                reset()
                for _ in range(steps):
                    loss = opt.step(inp)
            return loss

        run(2)                                                    # structure probe / verification, untimed
        _sync(dev)
        best, sync_best, loss = float("inf"), float("inf"), None
        for _ in range(3):
            if group is not None:
                torch.distributed.barrier()
            _sync(dev)
            t0 = time.perf_counter()
            loss = run(reps)
            _sync(dev)
            best = min(best, (time.perf_counter() - t0) / (reps * steps))
        for _ in range(3):                                        # the round-1 protocol: synchronise after every repetition
            reset()
            _sync(dev)
            t0 = time.perf_counter()
            for _ in range(steps):
                loss = opt.step(inp)
            _sync(dev)
            sync_best = min(sync_best, (time.perf_counter() - t0) / steps)
        return best, sync_best, float(loss), opt.linearization

    # default: the model's forward runs (dry) at every step, the reference's semantics; static=True: the caller's promise
    # that the residual program does not change, the model is not run
    best, sync_best, loss, path = measure(False)
    best_static, _, loss_static, _ = measure(True)
    world = 1 if group is None else torch.distributed.get_world_size(group)
    ach = 84.0 * B / best / 1e9
    traj = {"loss": [], "damping": [], "reject": []}
    if group is None:                       # untimed: one repetition read step by step (parity block against the CPU restatement)
        try:
            net = InvNet(init.clone())
            opt = pp.optim.LM(net, strategy=pp.optim.strategy.Constant(damping=1e-4))
            for _ in range(steps):
                traj["loss"].append(float(opt.step(inp)))
                traj["damping"].append(float(opt.param_groups[0]["damping"]))
                traj["reject"].append(int(opt.reject_count))
        except Exception as ex:
            traj["error"] = repr(ex)
    traj["initial_loss"], traj["residual_rows"] = l0, B
    return {"trajectory": traj, "algorithmic_bytes_per_step": 84 * B,
            "metric": "LM iters/sec (InvNet SE3, 1M independent problems per GPU)", "value": 1.0 / best, "unit": "LM steps/s",
            "static_model_value": 1.0 / best_static, "static_model_final_loss": loss_static,
            "problems_per_gpu": B, "n_gpus": world, "problem_steps_per_s": world * B / best, "path": path,
            "initial_loss": l0, "final_loss": loss, "steps_per_repetition": steps, "repetitions_in_flight": reps,
            "value_with_a_sync_per_repetition": 1.0 / sync_best,
            "roofline": _invnet_roofline(best, best_static, B, ach)}


def _invnet_roofline(best, best_static, B, ach):
    """configs[2] is at NEITHER roof: at kernel level the trial kernel issues 0.35 of the VALU peak and moves 0.51
    of the HBM peak by counted bytes, with 40 % of its wave-cycles on s_waitcnt; at step level the host adds its gap.  The block
    says so: `bound` = latency / occupancy, `frac` = the step's fraction of the 84 B / problem HBM roofline (the number SURVEY 8d
    prices the config with), the VALU-issue figure beside it."""
    valu = valu_roofline(["lm_se3inv_trial2", "lm_se3inv_finish"], best)
    return {"bound": "latency / occupancy: neither roof (kernel level: VALU issue 0.35, HBM 0.51 of peak by counted bytes, 40 % of "
                     "wave-cycles on s_waitcnt; the step adds the host's gap between launches)",
            "unit": "GB/s", "peak": HBM_PEAK_GBPS, "achieved": ach, "frac": ach / HBM_PEAK_GBPS,
            "frac_static_model": 84.0 * B / best_static / 1e9 / HBM_PEAK_GBPS,
            "algorithmic_bytes_per_step": 84 * B, "per": "LM step per GPU (SURVEY 8d C3: pose 28 r + input 28 r + pose 28 w)",
            "kernel": "lm_se3inv_trial2_kernel + lm_se3inv_finish_kernel (pplie_lm_se3inv_step_f32)",
            "valu": {k: valu.get(k) for k in ("achieved", "peak", "frac", "frac_ceiling_measured", "unit", "counter_source", "bound_note") if k in valu}}


def imu_rate(dev, B=4096, F=1024, reps=20, inner=16):
    """BASELINE configs[4]: IMUPreintegrator, B sequences x F steps, fp32, with and without covariance propagation
    (28 r + 40 w = 68 B / step, + 324 B / sequence for the covariance).  `inner` forwards are enqueued back to
    back per synchronisation (a sync costs ~40 us of launch + wake-up latency: amortised over 4 forwards it read as 11 us
    of each 70 us forward)."""
    import torch
    import pypose_amd as pp
    torch.manual_seed(0)
    dt = torch.full((B, F, 1), 0.005, device=dev)
    gyro = 0.1 * torch.randn(B, F, 3, device=dev)
    acc = torch.randn(B, F, 3, device=dev) + torch.tensor([0., 0., 9.81], device=dev)
    out = {"metric": "IMU pre-integration steps/s", "sequences": B, "steps": F, "unit": "steps/s"}
    for cov in (False, True):
        integ = pp.module.IMUPreintegrator(prop_cov=cov, reset=True).to(dev)
        f = lambda: integ(dt=dt, gyro=gyro, acc=acc)
        f()
        _sync(dev)
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            for _ in range(inner):
                f()
            _sync(dev)
            ts.append((time.perf_counter() - t0) / inner)
        t = sorted(ts)[len(ts) // 2]
        nbytes = 68.0 * B * F + (324.0 * B if cov else 0.0)
        out["with_covariance" if cov else "states_only"] = {
            "value": B * F / t, "ms": t * 1e3,
            "roofline": valu_roofline(["imu_integrate_multi"] + (["imu_cov_seg"] if cov else []), t, {
                "bound": "hbm", "unit": "GB/s", "peak": HBM_PEAK_GBPS, "achieved": nbytes / t / 1e9,
                "frac": nbytes / t / 1e9 / HBM_PEAK_GBPS, "algorithmic_bytes_per_launch": nbytes,
                "per": "module forward (68 B / step" + (" + 324 B / sequence)" if cov else ")")})}
    out["value"] = out["with_covariance"]["value"]
    return out


def _event_ms(dev, f, reps, warm=3, inner=1):
    """median HIP-event time of `f` (on torch's current stream: the stream every launch of the library uses); `inner` calls are
    enqueued back to back per event pair (a synchronisation per call exposes ~40 us of launch + wake-up latency)"""
    import torch
    for _ in range(warm):
        f()
    _sync(dev)
    ts = []
    if dev.type != "cuda":                     # (--standin dry run: plumbing only)
        for _ in range(reps):
            t0 = time.perf_counter(); f(); ts.append((time.perf_counter() - t0) * 1e3)
        return sorted(ts)[len(ts) // 2]
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            f()
        b.record(); _sync(dev)
        ts.append(a.elapsed_time(b) / inner)
    return sorted(ts)[len(ts) // 2]


def ops_10m_rates(dev, B=10_000_000, reps=20):
    """BASELINE configs[1] in full ("Batched SE3 Exp/Log/Adj, B = 10 M, fp32") as SURVEY 8(d) C2 lists it: Exp, Log, Adj forward,
    the two custom backwards, Jinvp, and the autograd chain x.Exp().Log().sum().backward(), each HIP-event timed at B rows with
    its algorithmic bytes per row (Exp / Log 52, Adj / Exp-bwd / Log-bwd / Jinvp 76, forward + backward pair 256)."""
    import torch
    import pypose_amd as pp
    from pypose_amd import _C
    torch.manual_seed(0)
    x = pp.randn_se3(B, device=dev).tensor().contiguous()
    torch.manual_seed(1)
    a = pp.randn_se3(B, device=dev).tensor().contiguous()
    X = _C.row_op("se3_exp_fwd", [x], (7,))[0]
    y = _C.row_op("se3_log_fwd", [X], (6,))[0]
    g7 = torch.randn(B, 7, device=dev)
    o6, o7 = torch.empty(B, 6, device=dev), torch.empty(B, 7, device=dev)
    kern = {"se3_exp_fwd": ([x], o7, 52), "se3_log_fwd": ([X], o6, 52), "se3_adj_fwd": ([X, a], o6, 76),
            "se3_exp_bwd": ([x, g7], o6, 76), "se3_log_bwd": ([y, a], o7, 76), "se3_jinvp_fwd": ([X, a], o6, 76)}
    out = {"metric": "BASELINE configs[1]: SE3 row operators at B = 10 M fp32, one launch each", "rows": B, "unit": "GB/s", "kernels": {}}
    for name, (ins, o, bpr) in kern.items():
        ms = _event_ms(dev, lambda: _C.row_op(name, ins, (o.shape[1],), out=[o]), reps)
        ach = B * bpr / ms / 1e6
        out["kernels"][name] = {"ms": ms, "bytes_per_row": bpr, "rows_per_s": B / ms * 1e3,
                                "roofline": {"bound": "hbm", "unit": "GB/s", "peak": HBM_PEAK_GBPS, "achieved": ach, "frac": ach / HBM_PEAK_GBPS}}
    del g7, o6, o7, y, X, a
    xg = pp.LieTensor(x, ltype=pp.se3_type).requires_grad_(True)

    def chain():
        xg.grad = None
        xg.Exp().Log().sum().backward()
    ms = _event_ms(dev, chain, max(5, reps // 2))
    ach = B * 256.0 / ms / 1e6
    out["fwd_bwd_chain"] = {"ms": ms, "pairs_per_s": B / ms * 1e3, "bytes_per_row": 256,
                            "roofline": {"bound": "hbm", "unit": "GB/s", "peak": HBM_PEAK_GBPS, "achieved": ach, "frac": ach / HBM_PEAK_GBPS,
                                         "per": "x.Exp().Log().sum().backward(): Exp 52 + Log 52 + Log-bwd 76 + Exp-bwd 76 B/row (SURVEY 8d C2); "
                                                "torch's own sum (24 B/row read) and the materialised ones cotangent (24 B/row written, "
                                                "24 read) ride on top and are NOT in the 256"}}
    fr = [k["roofline"]["frac"] for k in out["kernels"].values()]
    out["value"] = min(fr)
    out["slowest_kernel"] = min(out["kernels"], key=lambda k: out["kernels"][k]["roofline"]["frac"])
    del xg
    try:
        out["all_groups"] = ops_all_groups(dev, B, max(5, reps // 2))
    except Exception as e:                      # never lose the SE3 table over the wider one
        out["all_groups"] = {"error": repr(e)}
    return out


# widths of the four groups: (algebra, group)
_GROUP_W = {"so3": (3, 4), "se3": (6, 7), "sim3": (7, 8), "rxso3": (4, 5)}


def ops_all_groups(dev, B=10_000_000, reps=10):
    """What north_star names beyond SE3 Exp / Log: SO3 / SE3 / Sim3 / RxSO3 x {Exp, Log, Inv, Mul, Act, Adj} forward at B rows fp32,
    plus one fp64 row per group (Exp, Log), one launch each through the C ABI, HIP-event timed.  Algorithmic bytes per row =
    element size x (sum of input widths + sum of output widths).  Compact: {op: [ms, fraction of the 8 TB/s peak]}."""
    import torch
    import pypose_amd as pp
    from pypose_amd import _C
    res = {"rows": B, "unit": "[ms per launch, fraction of HBM peak]", "f32": {}, "f64": {}}
    gen = {"so3": pp.randn_so3, "se3": pp.randn_se3, "sim3": pp.randn_sim3, "rxso3": pp.randn_rxso3}
    for g, (da, dg) in _GROUP_W.items():
        for dtype, key, ops in ((torch.float32, "f32", ("exp", "log", "inv", "mul", "act", "adj")), (torch.float64, "f64", ("exp", "log"))):
            es = 4 if dtype == torch.float32 else 8
            torch.manual_seed(2)
            x = gen[g](B, device=dev, dtype=dtype).tensor().contiguous()
            X = _C.row_op(f"{g}_exp_fwd", [x], (dg,))[0]
            Y = a = p3 = None
            table = {"exp": ([x], dg), "log": ([X], da), "inv": ([X], dg)}
            if "mul" in ops:
                Y = _C.row_op(f"{g}_exp_fwd", [torch.roll(x, 1, 0).contiguous()], (dg,))[0]
                a = torch.randn(B, da, device=dev, dtype=dtype)
                p3 = torch.randn(B, 3, device=dev, dtype=dtype)
                table.update({"mul": ([X, Y], dg), "act": ([X, p3], 3), "adj": ([X, a], da)})
            for op in ops:
                ins, wo = table[op]
                o = torch.empty(B, wo, device=dev, dtype=dtype)
                name = f"{g}_{op}_fwd"
                ms = _event_ms(dev, lambda: _C.row_op(name, ins, (wo,), out=[o]), reps)
                bpr = es * (sum(t.shape[1] for t in ins) + wo)
                res[key][name] = [round(ms, 4), round(B * bpr / ms / 1e6 / HBM_PEAK_GBPS, 3)]
                del o
            del x, X, Y, a, p3, table
    res["min_frac_f32"] = min(v[1] for v in res["f32"].values())
    res["min_frac_f64"] = min(v[1] for v in res["f64"].values())
    res["below_0.65"] = sorted([k for k, v in res["f32"].items() if v[1] < 0.65] + [k + ":f64" for k, v in res["f64"].items() if v[1] < 0.65])
    return res


def imu_train_rate(dev, B=4096, F=1024, reps=10):
    """Training THROUGH the pre-integrator (examples/module/imu/imu_corrector.py:97) at BASELINE configs[4]'s shape: forward +
    backward of IMUPreintegrator(prop_cov=False) w.r.t. gyro and acc.  `integrator` times the integrator pair alone
    (torch.autograd.grad with given cotangents: pplie_imu_integrate + pplie_imu_integrate_bwd); `training_step` adds the
    example's loss (mse on pos + 5e2 x geodesic rotation error) and its own backward.  Beside each: the composed route -- the
    reference's formulation (Exp, log2(F) Hillis-Steele rounds of Mul, Act, Inv, two cumsums and their backward nodes) on the
    same HIP row kernels.  Algorithmic bytes per step: forward 28 r + 40 w, backward 28 (inputs) + 16 (rot) + 40 (cotangents)
    r + 24 w = 176 B."""
    import torch
    import pypose_amd as pp
    torch.manual_seed(0)
    dt = torch.full((B, F, 1), 0.005, device=dev)
    gyro = (0.1 * torch.randn(B, F, 3, device=dev)).requires_grad_(True)
    acc = (torch.randn(B, F, 3, device=dev) + torch.tensor([0., 0., 9.81], device=dev)).requires_grad_(True)
    gt_pos, gt_rot = torch.randn(B, F, 3, device=dev), pp.randn_SO3(B, F, device=dev)
    Wr, Wv, Wp = torch.randn(B, F, 4, device=dev), torch.randn(B, F, 3, device=dev), torch.randn(B, F, 3, device=dev)
    out = {"metric": "IMU pre-integration forward + backward, steps/s", "sequences": B, "steps": F, "unit": "steps/s"}
    nbytes = 176.0 * B * F
    grads = {}
    for route in ("fused", "composed"):
        integ = pp.module.IMUPreintegrator(prop_cov=False, reset=True).to(dev)
        integ.fused_backward = route == "fused"

        def pair():
            o = integ(dt=dt, gyro=gyro, acc=acc)
            return torch.autograd.grad([o["rot"].tensor(), o["vel"], o["pos"]], [gyro, acc], [Wr, Wv, Wp])

        def train():
            gyro.grad = acc.grad = None
            o = integ(dt=dt, gyro=gyro, acc=acc)
            loss = torch.nn.functional.mse_loss(o["pos"], gt_pos) + 5e2 * (gt_rot * o["rot"].Inv()).Log().norm(dim=-1).mean()
            loss.backward()
        n = reps if route == "fused" else max(3, reps // 3)
        ms_pair, ms_train = _event_ms(dev, pair, n, inner=4), _event_ms(dev, train, n, inner=4)
        grads[route] = [g.double() for g in pair()]
        out[route] = {"integrator": {"ms": ms_pair, "value": B * F / ms_pair * 1e3,
                                     "roofline": {"bound": "hbm", "unit": "GB/s", "peak": HBM_PEAK_GBPS, "achieved": nbytes / ms_pair / 1e6,
                                                  "frac": nbytes / ms_pair / 1e6 / HBM_PEAK_GBPS, "algorithmic_bytes_per_launch_pair": nbytes}},
                      "training_step": {"ms": ms_train, "value": B * F / ms_train * 1e3}}
    out["value"] = out["fused"]["integrator"]["value"]
    out["speedup_over_composed"] = {k: out["composed"][k]["ms"] / out["fused"][k]["ms"] for k in ("integrator", "training_step")}
    out["routes_agree_rel"] = max(float((a - b).abs().max() / b.abs().max()) for a, b in zip(grads["fused"], grads["composed"]))
    return out


def c1_latency(dev, B=1024):
    """BASELINE configs[0]: pp.randn_se3(1024).Exp().Log() forward + backward -- here the wall time of that call chain on
    the GPU (4 kernels; launch-latency bound at this size).  Bytes: 256 B / row forward + backward."""
    import torch
    import pypose_amd as pp
    torch.manual_seed(0)
    x = pp.randn_se3(B, device=dev, requires_grad=True)

    def fwd_bwd():
        x.grad = None
        x.Exp().Log().tensor().sum().backward()

    def fwd():
        with torch.no_grad():
            return x.Exp().Log()
    out = {"metric": "configs[0]: randn_se3(1024).Exp().Log() forward + backward", "B": B, "unit": "us per call chain"}
    for name, f in (("fwd_us", fwd), ("fwd_bwd_us", fwd_bwd)):
        for _ in range(50):
            f()
        _sync(dev)
        batches = []
        for _ in range(9):                                   # median of 9 batches of 100: a host hiccup does not set the figure
            t = time.perf_counter()
            for _ in range(100):
                f()
            _sync(dev)
            batches.append((time.perf_counter() - t) / 100 * 1e6)
        out[name] = sorted(batches)[len(batches) // 2]
        out[name + "_batches"] = [round(b, 1) for b in batches]
    out["value"] = out["fwd_bwd_us"]
    out["roofline"] = {"bound": "launch latency", "note": "1024 rows x 256 B = 0.26 MB per call chain: 33 ns at the HBM peak; "
                       "the figure is host dispatch + 4 dependent launches"}
    return out


def reproj_rate(dev, E=4_000_000, reps=10):
    """reprojection residual + closed-form Jacobian blocks of E (camera pose, point) observations in one
    kernel (pplie_se3_reproj_lin: 84 B read + 80 B written per observation), beside the same blocks from two batched backward
    sweeps of the unfused composition (SE3_Act kernel + tensor algebra)."""
    import torch
    import pypose_amd as pp
    from pypose_amd import _C
    from pypose_amd.optim import blocks as _blocks
    torch.manual_seed(0)
    X = pp.randn_SE3(E, sigma=0.3, device=dev).tensor().contiguous()
    p = (torch.randn(E, 3, device=dev) + torch.tensor([0, 0, 6.0], device=dev)).contiguous()
    K = torch.tensor([[500.0, 0, 320], [0, 500, 240], [0, 0, 1]], device=dev)
    cam = torch.cat([K.reshape(1, 9).expand(E, 9), torch.randn(E, 2, device=dev)], -1).contiguous()

    def med_ms(f, n):
        f(); _sync(dev)
        ts = []
        for _ in range(n):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); f(); b.record(); _sync(dev)
            ts.append(a.elapsed_time(b))
        return sorted(ts)[len(ts) // 2]

    ms = med_ms(lambda: _C.row_op("se3_reproj_lin", [X, p, cam], (2, 18)), reps)

    def sweeps():
        Xp = pp.SE3(X).requires_grad_(True)
        pr = p.clone().requires_grad_(True)
        r = pp.homo2cart(Xp.Act(pr) @ K.mT) - cam[:, 9:]
        return _blocks.jacobian_blocks([r], [Xp, pr])
    ms_auto = med_ms(sweeps, max(2, reps // 3))
    nbytes = 164.0 * E
    return {"metric": "reprojection linearisation (residual + closed-form blocks), observations/s", "unit": "observations/s",
            "observations": E, "value": E / (ms * 1e-3), "ms": ms, "autograd_blocks_ms": ms_auto,
            "roofline": {"bound": "hbm", "unit": "GB/s", "peak": HBM_PEAK_GBPS, "achieved": nbytes / ms / 1e6,
                         "frac": nbytes / ms / 1e6 / HBM_PEAK_GBPS, "algorithmic_bytes_per_launch": nbytes,
                         "per": "observation: pose 28 + point 12 + intrinsics / pixel 44 read, residual 8 + blocks 72 written"}}


def imu_sharded_rate(dev, rank, world, B=4096, F=1024):
    """configs[4] with the SEQUENCES sharded: every rank integrates its own B sequences, no collective."""
    import torch
    import torch.distributed as dist
    r = imu_rate(dev, B, F, reps=8)
    t = torch.tensor([r["with_covariance"]["ms"], r["states_only"]["ms"]], dtype=torch.float64, device=dev)
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    ms_cov, ms_plain = t.tolist()
    return {"metric": "IMU pre-integration steps/s, sequences sharded over the ranks (no collective)", "unit": "steps/s", "n_gpus": world,
            "sequences_per_gpu": B, "steps": F, "value": world * B * F / (ms_cov * 1e-3), "states_only_value": world * B * F / (ms_plain * 1e-3),
            "ms_max_over_ranks": {"with_covariance": ms_cov, "states_only": ms_plain}}


def pgo_sharded_lm_rate(dev, rank, world, nodes=100_000, edges=400_000, steps=3, reps=3, shard=None, exchange=None):
    """BASELINE configs[3]: pose-graph LM, 100k SE3 nodes / 400k relative-pose edges, sharded over the ranks --
    `LM(group=...)`, SURVEY.md section 8(e).  Same generator, solver and strategy as `pgo_lm_rate`.  Collective: every rank
    calls this; rank 0's figures are reported.  Not part of `value`.  shard / exchange None = the library's own choice
    (optim/posegraph.py resolve_shard_mode: node rows sharded over RCCL collectives for a graph of this size on GPUs; exchange="p2p": in-kernel peer stores)."""
    import torch
    import torch.distributed as dist
    import pypose_amd as pp
    e, rel, init = _pose_graph_problem(dev, nodes, edges)
    rel, init = rel.tensor().contiguous(), init.tensor().contiguous()
    for t in (e, rel, init):                      # one problem on every rank, whatever the device RNGs produced
        dist.broadcast(t, src=0)
    e_mine, rel_mine = e[rank::world].contiguous(), pp.SE3(rel[rank::world].contiguous())
    graph = _pose_graph_model(pp.SE3(init.clone()))
    solver = pp.optim.solver.PCG(tol=1e-4, maxiter=250)
    opt = pp.optim.LM(graph, solver=solver, strategy=pp.optim.strategy.TrustRegion(radius=1e4), group=dist.group.WORLD, shard=shard,
                      exchange=exchange)
    times, losses, its = [], [], []
    for rep in range(reps + 1):                   # repetition 0 (structure probe, kernel verification) is untimed
        graph.nodes.data.copy_(init)
        if hasattr(opt, "loss"):
            del opt.loss
        opt.param_groups[0].update(opt.strategy.defaults)
        _sync(dev)
        dist.barrier()
        t0 = time.perf_counter()
        losses, its = [], []
        for _ in range(steps):
            losses.append(float(opt.step((e_mine, rel_mine))))
            its.append(solver.iterations)
        _sync(dev)
        if rep:
            times.append((time.perf_counter() - t0) / steps)
    dt = sorted(times)[len(times) // 2]
    seen = torch.ones(1, device=dev)
    dist.all_reduce(seen)
    shard_eff, exch_eff = getattr(opt, "_shard_eff", shard), getattr(opt, "_exchange_eff", exchange)
    ns = getattr(opt, "_node_shards", {}).get("shard", (None, None))[1]
    p2p_state = getattr(ns, "p2p", None)
    its_mean = sum(its) / max(1, len(its))
    return {"metric": "LM iters/sec, pose graph 100k nodes / 400k edges sharded over the ranks (BASELINE configs[3])",
            "value": 1.0 / dt, "unit": "LM steps/s", "n_gpus": world, "ranks_seen": int(seen.item()), "nodes": nodes, "edges": edges,
            "edges_per_rank": int(e_mine.shape[0]), "path": opt.linearization, "losses": losses, "pcg_iterations": its, "ranks": world,
            "requested": {"shard": shard, "exchange": exchange}, "effective": {"shard": shard_eff, "exchange": exch_eff},
            "mode": getattr(opt, "_last_shard_mode", "replicated" if getattr(opt, "_last_replicated", False) else "edge-sharded"),
            "p2p_tables": (None if p2p_state is None else {"ok": bool(p2p_state.get("ok")), "epochs": int(p2p_state.get("epoch", 0)),
                                                             "error": repr(p2p_state.get("error")) if p2p_state.get("error") else None}),
            "us_per_pcg_iteration_incl_step_overheads": dt * 1e6 / max(1.0, its_mean),
            "exchange": ("in-kernel peer stores over xGMI (hipIpc-mapped tables, csrc/pcg_persist.hip): no collective per PCG iteration"
                         if exch_eff == "p2p" and shard_eff == "nodes" and (p2p_state or {}).get("ok", False)
                         else f"{dist.get_backend()} collectives (RCCL over xGMI on GPUs)"),
            "scales": ("no: every rank runs the whole solve (the blocks are all-gathered once per LM step)" if shard_eff == "edges" else
                       "the solve is sharded by node rows"),
            "repetitions_ms_per_step": [round(t * 1e3, 3) for t in times]}


# ---------------------------------------------------------------------------------------------------------------
def _r(x, nd=4):
    """a float rounded to `nd` significant digits (the summary must stay small)"""
    try:
        return float(f"{float(x):.{nd}g}")
    except Exception:
        return None


def _leg_summary(key, blk):
    """{v: value, u: unit, f: roofline fraction, b: bound, par: parity (error over tolerance, decisions equal), it: PCG iterations}"""
    if not isinstance(blk, dict) or "error" in blk:
        return {"error": (blk or {}).get("error", "missing")[:60]} if isinstance(blk, dict) else None
    roof = blk.get("roofline") or {}
    if key == "imu":
        roof = (blk.get("with_covariance") or {}).get("roofline") or {}
    if key == "imu_train":
        roof = ((blk.get("fused") or {}).get("integrator") or {}).get("roofline") or {}
    s = {"v": _r(blk.get("value")), "u": blk.get("unit")}
    bound = str(roof.get("bound", ""))
    s["b"] = bound.split(" ")[0].rstrip(":") if bound else None
    if roof.get("frac") is not None:
        s["f"] = _r(roof["frac"], 3)
    hb = roof.get("hbm") or {}
    if hb.get("frac") is not None:
        s["f_hbm"] = _r(hb["frac"], 3)
    if roof.get("us_per_pcg_iteration_incl_step_overheads") is not None:
        s["us_it"] = _r(roof["us_per_pcg_iteration_incl_step_overheads"], 3)
    if blk.get("pcg_iterations"):
        s["it"] = blk["pcg_iterations"]
    par = (blk.get("cpu_baseline") or {}).get("parity")
    if par:
        # (err_over_tol = |loss - reference loss| over the floor-aware tolerance of tests/test_fullsize_parity_gpu.py: <= 1 passes)
        s["par"] = {"err_over_tol": _r(par.get("loss_err_over_tolerance"), 2),
                    "dec_eq": bool(par.get("damping_equal")) and bool(par.get("reject_equal")), "n": par.get("steps_compared")}
    cb = blk.get("cpu_baseline") or {}
    if cb.get("value") is not None:
        s["cpu"] = _r(cb["value"], 3)
    # sharded legs (N > 1): ranks that took part, the mode that actually ran, the same work on one GPU
    if blk.get("ranks_seen") is not None:
        s["ranks"] = blk["ranks_seen"]
    eff = blk.get("effective") or {}
    if eff:
        s["mode"] = f"{eff.get('shard')}/{eff.get('exchange')}"
    if roof.get("us_per_pcg_iteration_incl_step_overheads") is None and blk.get("us_per_pcg_iteration_incl_step_overheads") is not None:
        s["us_it"] = _r(blk["us_per_pcg_iteration_incl_step_overheads"], 3)
    if isinstance(blk.get("one_gpu_equivalent"), dict):
        s["one_gpu"] = _r(blk["one_gpu_equivalent"].get("value"), 4)
    if blk.get("speedup_vs_one_gpu") is not None:
        s["x"] = _r(blk["speedup_vs_one_gpu"], 3)
    return {k: v for k, v in s.items() if v is not None}


def _lift_second_half(out):
    """The driver's record keeps the contract keys (`config`, `roofline`, `cpu_baseline` whole) and the last ~2000 characters of
    the line: BASELINE.json's metric has a second half ("LM iters/sec (PGO 10k poses)") and four more configs, so their figures go
    (1) to the top level as `value_lm_pgo_10k` / `roofline_lm_pgo_10k`, (2) into `config.metric_second_half`, and (3) into a
    compact `summary` that is the LAST key of the line (one entry per leg: value, unit, roofline fraction and bound, parity,
    PCG iterations, CPU baseline value)."""
    pgo = out.get("lm_pgo") if isinstance(out.get("lm_pgo"), dict) else None
    if pgo and "value" in pgo:
        roof = pgo.get("roofline") or {}
        out["value_lm_pgo_10k"] = pgo["value"]
        out["unit_lm_pgo_10k"] = "LM steps/s (10k poses / 40k edges, PCG tol 1e-4, TrustRegion, fp32)"
        out["roofline_lm_pgo_10k"] = {k: roof.get(k) for k in ("bound", "unit", "us_per_lm_step", "mean_pcg_iterations",
                                                               "us_per_pcg_iteration_incl_step_overheads", "marginal_us_per_iteration",
                                                               "exchange_floor_us") if k in roof}
        par = (pgo.get("cpu_baseline") or {}).get("parity") or {}
        out["config"]["metric_second_half"] = {
            "metric": pgo.get("metric"), "value": _r(pgo["value"], 5), "unit": "LM steps/s", "pcg_iterations": pgo.get("pcg_iterations"),
            "us_per_pcg_iteration": _r(roof.get("us_per_pcg_iteration_incl_step_overheads"), 3), "bound": "latency",
            "parity_err_over_tolerance": _r(par.get("loss_err_over_tolerance"), 2),
            "parity_protocol": "loss/damping/reject sequence vs the CPU restatement of the reference's loop on the same instance; tolerance is "
                               "floor-aware (inexact PCG, tol 1e-4: 1e-3); the 1e-5 bar is asserted on the tight-solve twins (tests/test_fullsize_parity_gpu.py)",
            "decisions_equal": (bool(par.get("damping_equal")) and bool(par.get("reject_equal"))) if par else None,
            "cpu_baseline_value": _r((pgo.get("cpu_baseline") or {}).get("value"), 3)}
    summ = {}
    for key in ("c1", "ops_10m", "lm_invnet", "lm_pgo", "lm_pgo_100k", "imu", "imu_train", "ba_reproj",
                "lm_invnet_sharded", "imu_sharded", "lm_pgo_replicated", "lm_pgo_node_sharded", "lm_pgo_100k_one_gpu"):
        if key in out:
            summ[key] = _leg_summary(key, out[key])
    ops = out.get("ops_10m") if isinstance(out.get("ops_10m"), dict) else None
    if ops and "kernels" in ops:
        summ["ops_10m"] = {"se3_f": {k.replace("se3_", ""): _r(v["roofline"]["frac"], 3) for k, v in ops["kernels"].items()},
                           "chain_f": _r((ops.get("fwd_bwd_chain") or {}).get("roofline", {}).get("frac"), 3)}
        ag = ops.get("all_groups") or {}
        if "f32" in ag:
            summ["ops_10m"].update({"min_f32": ag.get("min_frac_f32"), "min_f64": ag.get("min_frac_f64"), "lt065": ag.get("below_0.65")})
    if isinstance(out.get("lm_pgo_sharded"), dict):
        summ["lm_pgo_sharded"] = "after this line: stderr PPLIE_BENCH_POSTLINE" if "deferred" in out["lm_pgo_sharded"] else "skipped"
    head = {"pairs_per_s": _r(out.get("value"), 5), "f": _r((out.get("roofline") or {}).get("frac"), 3), "n_gpus": out.get("n_gpus")}
    out.pop("summary", None)
    out["summary"] = {"headline": head, **summ}        # LAST key: lands in the tail of the line


def _self_launch(a):
    """`python bench.py --gpus N` with N > 1 and no launcher: re-execute under torch.distributed.run, one process per GPU."""
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env["PPLIE_BENCH_SELF_LAUNCHED"] = "1"
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={a.gpus}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    os.execvpe(sys.executable, cmd, env)


_REAL_STDOUT = None


def _claim_stdout():
    """The contract is ONE JSON line on stdout.  RCCL prints a version banner to stdout through C stdio (it lands before or
    after the line depending on buffering), other libraries may chat too: fd 1 is pointed at stderr for the whole run and
    the line goes to a private duplicate of the real stdout."""
    global _REAL_STDOUT
    if _REAL_STDOUT is None:
        sys.stdout.flush()
        _REAL_STDOUT = os.dup(1)
        os.dup2(2, 1)


def _emit_line(text):
    if _REAL_STDOUT is None:
        print(text, flush=True)
    else:
        os.write(_REAL_STDOUT, (text + "\n").encode())


LINE_LIMIT = 12_000            # bytes: the driver's record keeps a parsed copy of the line only while it stays small (r05 lost it at 22 KB)
_LINE_KEYS = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
              "dtype", "data", "ranks_seen", "config", "roofline", "cpu_baseline", "value_lm_pgo_10k", "unit_lm_pgo_10k",
              "roofline_lm_pgo_10k", "sharded_legs", "instances_error")


def _detail_path():
    p = os.environ.get("PPLIE_BENCH_DETAIL")
    if p:
        return p
    d = os.path.join(ROOT, "gpurun_out")
    try:
        os.makedirs(d, exist_ok=True)
    except OSError:
        d = ROOT
    return os.path.join(d, "bench_legs.json")


def _compact(out, detail):
    """The ONE stdout line: the contract keys, `config` (with the metric's second half), `roofline`, `cpu_baseline` and the
    per-leg `summary` -- nothing else.  Every leg's full block lives in the side file `detail`."""
    line = {k: out[k] for k in _LINE_KEYS if k in out}
    cb = line.get("cpu_baseline")
    if isinstance(cb, dict):
        cb = {k: v for k, v in cb.items() if k in ("value", "unit", "cores", "host_cores", "kind", "sample", "error")}
        if isinstance(cb.get("sample"), str) and len(cb["sample"]) > 400:
            cb["sample"] = cb["sample"][:397] + "..."
        line["cpu_baseline"] = cb
    line["detail"] = detail
    line["summary"] = out.get("summary")                    # LAST key
    text = json.dumps(line)
    if len(text) > LINE_LIMIT:                              # never: the summary is a few hundred bytes per leg -- but the line must parse
        line["summary"] = {"headline": (out.get("summary") or {}).get("headline"), "truncated": "see detail"}
        text = json.dumps(line)
    return text


def _finish(out):
    """full record -> side file (+ stderr); compact line -> stdout"""
    full = json.dumps(out)
    path = _detail_path()
    try:
        with open(path, "w") as f:
            f.write(full + "\n")
    except OSError as e:
        path = f"stderr only ({e!r})"
    sys.stderr.write("PPLIE_BENCH_DETAIL " + full + "\n")
    sys.stderr.flush()
    if os.path.isabs(path) and path.startswith(ROOT + os.sep):
        path = os.path.relpath(path, ROOT)
    _emit_line(_compact(out, path))


DUMP_BYTES = 60_000_000         # --dump-outputs: all files of all ranks together stay below this


def _dump_outputs(d, rank, world, arrays):
    """--dump-outputs DIR: the arrays the last timed step handed back, as DIR/<name>.npy (DIR/<name>_rank<r>.npy with more than
    one rank), float32 or float64.  All arrays have one row per input row; when they exceed DUMP_BYTES the same sorted sample of
    rows (numpy default_rng(0), so the same rows in every run with the same arguments) is kept of each."""
    import numpy as np
    import torch
    os.makedirs(d, exist_ok=True)
    ts = {}
    for name, v in arrays.items():
        t = (v.tensor() if hasattr(v, "tensor") else v).detach()
        ts[name] = t if t.dtype in (torch.float32, torch.float64) else t.to(torch.float32)
    rows = next(iter(ts.values())).shape[0]
    row_bytes = sum(t[0].numel() * t.element_size() for t in ts.values())
    keep = min(rows, DUMP_BYTES // (world * row_bytes))
    idx = None
    if keep < rows:
        idx = torch.from_numpy(np.sort(np.random.default_rng(0).choice(rows, keep, replace=False)))
    for name, t in ts.items():
        part = t if idx is None else t[idx.to(t.device)]
        np.save(os.path.join(d, name + (f"_rank{rank}" if world > 1 else "") + ".npy"), part.cpu().numpy())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rows", type=int, default=10_000_000, help="rows per GPU (BASELINE configs[1]: 10M)")
    ap.add_argument("--full", action="store_true",
                    help="after the headline also run everything else: the legs of the other BASELINE configs, the CPU baselines, "
                         "with N > 1 the sharded legs; writes the side file of full blocks.  Off: headline only")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps write what the last timed step computed (X = x.Exp(), y = X.Log(); a fixed seeded "
                         "sample of rows when larger than the budget) as DIR/<name>.npy")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: leave the CPU baselines out")
    ap.add_argument("--no-secondary", action="store_true", help="with --full: leave the other legs out")
    ap.add_argument("--backend", default="nccl", choices=["nccl", "gloo"],
                    help="gloo + --standin: CPU dry run of the multi-process plumbing (tests/test_bench_launch.py)")
    ap.add_argument("--standin", action="store_true",
                    help="TEST ONLY: run on CPU tensors with the oracle stand-in of the HIP library (tests/oracle_backend.py); "
                         "nothing it prints is a measurement")
    a = ap.parse_args()
    if a.steps < 1:
        ap.error("--steps must be at least 1")
    if a.gpus > 1 and "WORLD_SIZE" not in os.environ:
        _self_launch(a)
    _claim_stdout()
    import torch

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    launched = "WORLD_SIZE" in os.environ and "RANK" in os.environ      # torch.distributed.run (also with one rank)
    standin = a.standin
    if standin:
        assert a.backend == "gloo", "--standin is the CPU dry run: use --backend gloo"
        from tests.oracle_backend import oracle_row_op
        from pypose_amd import _C as _C0
        _C0.set_backend_for_testing(oracle_row_op)
        dev = torch.device("cpu")
    else:
        dev = torch.device("cuda", local)
        torch.cuda.set_device(dev)
    if launched:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        if a.backend == "nccl":
            dist.init_process_group("nccl", device_id=dev)
        else:
            dist.init_process_group("gloo")
    assert world == a.gpus, f"--gpus {a.gpus} but WORLD_SIZE={world}"

    import pypose_amd as pp
    from pypose_amd import _C
    assert standin or _C._test_backend is None

    B = a.rows
    torch.manual_seed(rank)
    x = pp.randn_se3(B, device=dev)          # [B,6] fp32, resident in HBM before timing starts

    def step():
        X = x.Exp()
        return X.Log()

    for _ in range(a.warmup):
        y = step()
    _sync(dev)

    # HIP events bracket both kernels on every `EV`-th step of the timed region (default: every step).  Each record is
    # a packet in the stream: on every step they cost ~3% of `value`, but bracketing only some steps makes exactly
    # those launches slower (92-96 us instead of 90 for Log), so the per-kernel figure is taken on all of them
    EV = max(1, int(os.environ.get("PPLIE_BENCH_EVENT_STRIDE", "1")))
    ev = {} if standin else {k: [torch.cuda.Event(enable_timing=True) for _ in range(3)] for k in range(0, a.steps, EV)}

    def barrier():
        if launched:
            import torch.distributed as dist
            dist.barrier()

    barrier()
    _sync(dev)
    t0 = time.perf_counter()
    for k in range(a.steps):
        e = ev.get(k)
        if e is None:
            X = x.Exp()
            y = X.Log()
        else:
            e[0].record()
            X = x.Exp()
            e[1].record()
            y = X.Log()
            e[2].record()
    _sync(dev)
    barrier()
    elapsed = time.perf_counter() - t0

    t = torch.tensor([elapsed], dtype=torch.float64, device=dev)
    if launched:
        import torch.distributed as dist
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
    elapsed = t.item()
    seen = torch.ones(1, dtype=torch.float64, device=dev)        # every rank that took part in the timed region adds one
    if launched:
        dist.all_reduce(seen)
    ranks_seen = int(seen.item())
    if a.dump_outputs:
        _dump_outputs(a.dump_outputs, rank, world, {"exp": X, "log": y})

    out = None
    if rank == 0:
        if ev:
            ms_exp = sum(e[0].elapsed_time(e[1]) for e in ev.values()) / len(ev)
            ms_log = sum(e[1].elapsed_time(e[2]) for e in ev.values()) / len(ev)
        else:
            ms_exp = ms_log = elapsed / a.steps * 1e3 / 2
        dom, ms_dom = ("se3_log_fwd", ms_log) if ms_log >= ms_exp else ("se3_exp_fwd", ms_exp)
        achieved = B * BYTES_PER_ROW[dom] / (ms_dom * 1e-3) / 1e9
        traffic = None
        pmcj = _pmc("pmc_traffic")
        traffic = pmcj.get(dom)
        out = {
            "metric": "batched SE3 Exp+Log ops/sec (BASELINE metric, first half; second half under lm_pgo)",
            "value": world * B * a.steps / elapsed,
            "unit": "SE3 Exp+Log pairs/s", "n_gpus": world, "steps": a.steps, "warmup": a.warmup,
            "ms_per_step": elapsed / a.steps * 1e3, "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": "f32", "data": "synthetic" if not standin else "DRY RUN on the CPU stand-in: not a measurement",
            "ranks_seen": ranks_seen,
            "config": {"workload": "se3_explog_b10m (BASELINE configs[1]: batched SE3 Exp then Log, fp32, forward)",
                       "rows_per_gpu": B, "parallelism": f"rows sharded x{world}, no collective",
                       "ranks": world, "collective_backend": (a.backend if launched else None),
                       "launch": "self-launched torch.distributed.run" if os.environ.get("PPLIE_BENCH_SELF_LAUNCHED") else
                                 ("torch.distributed.run" if launched else "single process")},
            "roofline": {"bound": "hbm", "kernel": f"rowmap_lds_kernel<{dom}> (pplie_{dom}_f32)",
                         "achieved": achieved, "peak": HBM_PEAK_GBPS, "unit": "GB/s", "frac": achieved / HBM_PEAK_GBPS,
                         "traffic": traffic, "traffic_source": (f"profiles/pmc_traffic.json ({pmcj.get('_stamp', 'unstamped')}): rocprofv3 --pmc passes of an "
                                            "earlier run of this kernel on this workload; not collected in this run") if traffic is not None else None,
                         "algorithmic_bytes_per_launch": B * BYTES_PER_ROW[dom],
                         "avg_launch_ms": ms_dom, "timed_launches": len(ev), "other_kernel_ms": {"se3_exp_fwd": ms_exp, "se3_log_fwd": ms_log}},
        }
    import gc
    gc.collect()
    gc.freeze()                   # (a gen-2 collection with torch loaded is a 40-70 ms pause)
    small = standin                # the dry run shrinks every leg: it checks plumbing, not speed
    instances = {}
    if world == 1 and a.full and not a.no_secondary and rank == 0:
        x = y = X = None                      # (the headline's 0.8 GB go back to the allocator before the 10 M-row legs)
        def make_instances():
            # (after the latency-sensitive legs: building the host instances runs multi-threaded CPU kernels whose worker
            #  threads keep spinning for a while and would sit in c1's microseconds)
            try:
                instances.update(_host_instances(small, standin))
            except Exception as e:
                out["instances_error"] = repr(e)
            return None
        legs = (("c1", lambda: c1_latency(dev)),
                ("ops_10m", lambda: ops_10m_rates(dev, 4000 if small else 10_000_000, reps=2 if small else 20)),
                ("_instances", make_instances),
                ("lm_invnet", lambda: invnet_lm_rate(dev, B=2000 if small else 1_000_000, reps=2 if small else 40,
                                                     problem=instances.get("lm_invnet"))),
                ("lm_pgo", lambda: pgo_lm_rate(dev, *((60, 150) if small else (10_000, 40_000)), reps=1 if small else 25,
                                               problem=instances.get("lm_pgo"))),
                ("lm_pgo_100k", lambda: pgo_lm_rate(dev, *((80, 200) if small else (100_000, 400_000)), reps=1 if small else 9,
                                                    with_static=False, problem=instances.get("lm_pgo_100k"))),
                ("imu", lambda: imu_rate(dev, *((8, 64) if small else (4096, 1024)), reps=2 if small else 20)),
                ("imu_train", lambda: imu_train_rate(dev, *((8, 64) if small else (4096, 1024)), reps=2 if small else 10)),
                ("ba_reproj", lambda: reproj_rate(dev, 2000 if small else 4_000_000, reps=2 if small else 10)))
        for key, fn in legs:
            try:
                res = fn()
                if res is not None:
                    out[key] = res
            except Exception as e:    # never lose the headline line over a secondary figure
                out[key] = {"error": repr(e)}
    if world == 1 and a.full and not a.no_cpu_baseline and rank == 0 and not standin:
        out["cpu_baseline"] = cpu_baseline()
        if not a.no_secondary:
            try:
                per_leg = leg_cpu_baselines(int(out["cpu_baseline"].get("cores") or 8) if out["cpu_baseline"].get("kind") == "reference" else 8,
                                            instances, out)
            except Exception as e:
                per_leg = {"error": repr(e)}
            for key, blk in per_leg.items():
                if isinstance(out.get(key), dict):
                    out[key]["cpu_baseline"] = blk
    if world == 1 and a.full and standin and rank == 0:
        dt, _ = _cpu_worker((0, 20_000))           # the block's shape in the dry run (one process, 20k rows of the numpy port)
        out["cpu_baseline"] = {"value": 20_000 / dt, "unit": "SE3 Exp+Log pairs/s", "cores": 1, "kind": "port",
                               "sample": "DRY RUN: 20000 rows of oracle/lie_np.py se3_exp_fwd+se3_log_fwd in this process"}
    if rank == 0 and out is not None:
        _lift_second_half(out)
    sharded = a.full and launched and not a.no_secondary and (world > 1 or os.environ.get("PPLIE_BENCH_SHARDED") == "1")
    if sharded:
        # every rank takes part; a watchdog keeps the headline line if a collective wedges (nothing in the timed
        # region above depends on this)
        import threading
        import torch.distributed as dist
        finished, printed = threading.Event(), threading.Lock()

        def emit():
            if printed.acquire(blocking=False) and rank == 0:
                try:
                    _lift_second_half(out)                    # (again: the sharded legs are in, the summary stays the last key)
                except Exception:
                    pass
                _finish(out)

        def watchdog():
            if not finished.wait(float(os.environ.get("PPLIE_BENCH_SHARDED_TIMEOUT", "240"))):
                if rank == 0:
                    out["sharded_legs"] = "timed out"
                emit()
                os._exit(0)

        threading.Thread(target=watchdog, daemon=True).start()
        legs = (("lm_invnet_sharded", lambda: invnet_lm_rate(dev, B=2000 if small else 1_000_000, reps=2 if small else 40,
                                                             group=dist.group.WORLD)),
                ("imu_sharded", lambda: imu_sharded_rate(dev, rank, world, *((8, 64) if small else (4096, 1024)))),
                # the two modes that only use RCCL collectives: the replicated solve (the fallback) and node shards over collectives
                ("lm_pgo_replicated", lambda: pgo_sharded_lm_rate(dev, rank, world, *((80, 200) if small else (100_000, 400_000)),
                                                                  reps=1 if small else 2, shard="edges", exchange="rccl")),
                ("lm_pgo_node_sharded", lambda: pgo_sharded_lm_rate(dev, rank, world, *((80, 200) if small else (100_000, 400_000)),
                                                                    reps=1 if small else 2, shard="nodes", exchange="rccl")))
        for key, fn in legs:
            try:
                res = fn()
            except Exception as e:
                res = {"error": repr(e)}
            if rank == 0:
                out[key] = res
        # The OPT-IN exchange of the node-sharded solve -- p and the partial sums stored straight into the peers' tables from inside
        # one persistent kernel per GPU (hipIpc-mapped memory over xGMI; LM(exchange="p2p"), the library's default until round 6) --
        # has never run across two physical GPUs in the builder's hands (ranks as processes on one GPU only).  A GPU memory fault
        # there would abort the job before the line is out, so the line goes out FIRST (with a note of what follows) and the leg's
        # result is written to stderr and to bench_p2p_leg.json beside this file afterwards.
        # One-GPU equivalents, so that an N = 1 / N = 8 ratio falls out of this ONE line: the weak-scaling legs (problems / sequences
        # per rank fixed) scale against value / ranks; configs[3] is ONE graph whatever N is (strong scaling): rank 0 runs the
        # un-sharded single-GPU path on it while the other ranks wait at the barrier.
        try:
            one = pgo_lm_rate(dev, *((80, 200) if small else (100_000, 400_000)), reps=1 if small else 5, with_static=False) if rank == 0 else None
        except Exception as e:
            one = {"error": repr(e)}
        dist.barrier()
        if rank == 0:
            out["lm_pgo_100k_one_gpu"] = {k: one.get(k) for k in ("value", "unit", "pcg_iterations", "losses", "error") if k in one}
            for key in ("lm_invnet_sharded", "imu_sharded"):
                if isinstance(out.get(key), dict) and "value" in out[key]:
                    out[key]["one_gpu_equivalent"] = {"value": out[key]["value"] / world, "note": "weak scaling: per-rank work is fixed, "
                                                      "the aggregate over ranks_seen ranks divided by their number"}
            for key in ("lm_pgo_replicated", "lm_pgo_node_sharded"):
                if isinstance(out.get(key), dict) and "value" in out[key] and one and one.get("value"):
                    out[key]["one_gpu_equivalent"] = {"value": one["value"], "note": "strong scaling: the same 100k / 400k graph on rank 0 "
                                                      "alone (single-GPU path, this run)"}
                    out[key]["speedup_vs_one_gpu"] = out[key]["value"] / one["value"]
        post = os.environ.get("PPLIE_BENCH_P2P_LEG", "1") != "0"
        if rank == 0:
            out["lm_pgo_sharded"] = {"deferred": "runs after this line: LM(group=, shard='nodes', exchange='p2p') (node shards + in-kernel peer stores, opt-in); "
                                                 "result on stderr as 'PPLIE_BENCH_POSTLINE {json}' and in bench_p2p_leg.json"} if post \
                else {"skipped": "PPLIE_BENCH_P2P_LEG=0"}
        finished.set()
        emit()
        if post:
            def post_watchdog():                          # (the line is out: a wedged peer exchange must not hold the job)
                time.sleep(float(os.environ.get("PPLIE_BENCH_P2P_TIMEOUT", "150")))
                if rank == 0:
                    sys.stderr.write('PPLIE_BENCH_POSTLINE {"lm_pgo_sharded": {"error": "timed out"}}\n')
                    sys.stderr.flush()
                os._exit(0)
            threading.Thread(target=post_watchdog, daemon=True).start()
            try:
                res = pgo_sharded_lm_rate(dev, rank, world, *((80, 200) if small else (100_000, 400_000)), reps=1 if small else 3,
                                          shard="nodes", exchange="p2p")
            except Exception as e:
                res = {"error": repr(e)}
            if rank == 0:
                if isinstance(res, dict) and "value" in res and isinstance(out.get("lm_pgo_100k_one_gpu"), dict) and out["lm_pgo_100k_one_gpu"].get("value"):
                    res["one_gpu_equivalent"] = {"value": out["lm_pgo_100k_one_gpu"]["value"], "note": "the same graph on rank 0 alone, this run"}
                    res["speedup_vs_one_gpu"] = res["value"] / out["lm_pgo_100k_one_gpu"]["value"]
                txt = json.dumps({"lm_pgo_sharded": res})
                sys.stderr.write("PPLIE_BENCH_POSTLINE " + txt + "\n")
                sys.stderr.flush()
                try:
                    with open(os.path.join(ROOT, "bench_p2p_leg.json"), "w") as f:
                        f.write(txt + "\n")
                except OSError:
                    pass
    elif rank == 0 and a.full:
        _finish(out)
    elif rank == 0:
        _emit_line(_compact(out, None))         # headline only: the line is the whole record, no side file
    if launched:
        import torch.distributed as dist
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
