"""One bipartite problem from random blocks for the point-eliminated PCG (tests/test_ba_schur_*.py), with its dense fp64
reference.  Track lengths cover every path of csrc/ba_schur.hip: lane groups of 1..64 lanes (0, 1, 2, 5, 63, 64 observations),
the workgroup path (65), several chunks of 256 (300, 700, 1500); camera 0 holds more than one work item of 1024 observations
and camera 6 has none.  The point index is shuffled, the camera index random."""
import torch

from pypose_amd.optim import multigraph

NC, TRACKS = 7, [0, 1, 2, 5, 63, 64, 65, 300, 700, 1500]
KEPT = {6: (6,), 9: (3, 6), 5: (2, 3)}


class Opt:
    group = None


def problem(mb, seed=0):
    """fp64 host tensors: kept blocks (one per kept slot), eliminated blocks Ja [E, 2, 3], R, indices, a random positive shift"""
    g = torch.Generator().manual_seed(seed)
    tracks = torch.tensor(TRACKS + torch.randint(1, 7, (50,), generator=g).tolist())
    Np = tracks.numel()
    pidx = torch.repeat_interleave(torch.arange(Np), tracks)
    pidx = pidx[torch.randperm(pidx.numel(), generator=g)]
    E = pidx.numel()
    cidx = torch.multinomial(torch.tensor([0.5, 0.1, 0.1, 0.1, 0.1, 0.1, 0.0]), E, replacement=True, generator=g)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    Jk, Ja, R = [rnd(E, 2, m) for m in KEPT[mb]], rnd(E, 2, 3), rnd(E, 2)
    # dense J over [kept unknowns | eliminated unknowns]
    J = torch.zeros(2 * E, NC * mb + Np * 3, dtype=torch.float64)
    rows = torch.arange(2 * E).view(E, 2, 1)
    J[rows, (cidx * mb).view(E, 1, 1) + torch.arange(mb)] = torch.cat(Jk, -1)
    J[rows, NC * mb + (pidx * 3).view(E, 1, 1) + torch.arange(3)] = Ja
    H = J.T @ J
    shift = 1e-2 * H.diagonal().clamp_min(1.0) * (0.5 + torch.rand(H.shape[0], generator=g, dtype=torch.float64))
    return dict(mb=mb, Np=Np, E=E, cidx=cidx, pidx=pidx, Jk=Jk, Ja=Ja, R=R, J=J, shift=shift)


def reference(P, shift=None):
    """dense fp64: S, b_S, the back-substitution and the full damped system (H, g) in [kept | eliminated] order"""
    n = NC * P["mb"]
    H = P["J"].T @ P["J"] + torch.diag(P["shift"] if shift is None else shift)
    g = P["J"].T @ P["R"].reshape(-1)
    U, W, V = H[:n, :n], H[:n, n:], H[n:, n:]
    Vinv = torch.linalg.inv(V)
    S = U - W @ Vinv @ W.T
    return dict(H=H, g=g, S=S, bS=-(g[:n] - W @ Vinv @ g[n:]), back=lambda xc: -Vinv @ (g[n:] + W.T @ xc.reshape(-1)))


def linearization(P, dtype, device, W=None):
    """(lin, shift per parameter): parameters = the kept slots' (NC rows) then the points"""
    t = lambda x: x.to(dtype).to(device)
    widths = list(KEPT[P["mb"]]) + [3]
    params = [torch.zeros(NC if k < len(widths) - 1 else P["Np"], w, dtype=dtype, device=device) for k, w in enumerate(widths)]
    cidx, pidx = P["cidx"].to(device), P["pidx"].to(device)
    slots = [(k, cidx, t(J)) for k, J in enumerate(P["Jk"])] + [(len(widths) - 1, pidx, t(P["Ja"]))]
    lin = multigraph.MultiGraphLinearization(Opt(), None if W is None else t(W), t(P["R"]), params, slots)
    sc = t(P["shift"][:NC * P["mb"]]).view(NC, P["mb"])
    shift, off = [], 0
    for w in widths[:-1]:
        shift.append(sc[:, off:off + w].contiguous())
        off += w
    shift.append(t(P["shift"][NC * P["mb"]:]).view(P["Np"], 3))
    return lin, shift


def operators(ops, P, xc):
    """the five checked quantities of one implementation, as flat fp64 host tensors in the reference's layout"""
    mb = P["mb"]
    Scc, Minv = ops.blocks()
    x = xc.to(Scc.dtype).to(Scc.device).view(NC, mb)
    out = dict(Sx=ops.S(x), bS=ops.b_S(), Scc=Scc, Minv_x=(Minv @ x.unsqueeze(-1)), back=ops.back(x))
    return {k: v.double().cpu().reshape(-1) for k, v in out.items()}


def reference_operators(P, xc):
    mb = P["mb"]
    ref = reference(P)
    Scc = torch.stack([ref["S"][c * mb:(c + 1) * mb, c * mb:(c + 1) * mb] for c in range(NC)])
    return dict(Sx=ref["S"] @ xc, bS=ref["bS"], Scc=Scc.reshape(-1), Minv_x=torch.linalg.solve(Scc, xc.view(NC, mb, 1)).reshape(-1),
                back=ref["back"](xc))
