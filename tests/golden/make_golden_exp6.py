"""Golden vectors of exp-6 (race debiasing), produced by EXECUTING the reference's own code.

Run in the build container only (needs /root/reference); the outputs are committed:
  * reference_cli_exp6.json -- exp-6's ``parse_args`` defaults and each YAML overlay, in the shape of reference_cli_multi.json;
  * reference_exp6_targets.npz -- the lifted ``generate_dynamic_targets_race`` for a set of global face counts N: the composition
    table the reference kept (ordered compositions and their weights, recorded as it enters the transport loop), the float64
    input probabilities (fp32-representable values, some -1 rows), the targets and the fp64 uncertainties.

POT is not installed here, so three names of the lifted function's namespace are stand-ins: ``ot.dist`` (euclidean distance of each
probability vector to the one-hot corners, the formula of fairness.mc_transport_problem), ``ot.emd`` (scipy's assignment on the
capacity-replicated cost matrix: unit sources and integer sinks have an integral optimum) and ``itertools.zip_longest`` (records the
kept table it is handed).  No reference source text is stored: only inputs and outputs.
"""
import itertools
import json
import os
import sys
import types

import numpy as np
import torch
import yaml

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import lift  # noqa: E402

EXP6 = "/root/reference/exp-6-debias-race"
NS = [0, 1, 2, 3, 4, 7, 8, 16, 31, 32, 35, 36, 40, 64]


def _dist(x1, x2, metric="euclidean", p=None):
    assert metric == "euclidean"
    x1, x2 = np.asarray(x1, dtype=np.float64), np.asarray(x2, dtype=np.float64)
    M = np.zeros((x1.shape[0], x2.shape[0]))
    for j in range(x2.shape[0]):
        sq = np.zeros(x1.shape[0])
        sq += ((x1 - x2[j]) ** 2).sum(axis=1)
        M[:, j] = np.sqrt(sq)
    return M


def _emd(a, b, M):
    from scipy.optimize import linear_sum_assignment
    N, K = M.shape
    cols = np.repeat(np.arange(K), np.asarray(b, dtype=np.int64))
    assert len(cols) == N and np.all(np.asarray(a) == 1)
    T = np.zeros((N, K))
    if N:
        r, c = linear_sum_assignment(M[:, cols])
        T[r, cols[c]] = 1.0
    return T


def cli_golden():
    pa = lift(["parse_args"], ref=f"{EXP6}/1-main-debias.py")["parse_args"]
    os.environ.pop("LOCAL_RANK", None)
    e = dict(defaults=vars(pa([])))
    cdir = f"{EXP6}/configs"
    for f in sorted(os.listdir(cdir)):
        if f.endswith(".yaml") and "compute_environment" not in yaml.safe_load(open(os.path.join(cdir, f))):   # skip the accelerate launcher config
            e[f] = dict(yaml=yaml.safe_load(open(os.path.join(cdir, f))), args=vars(pa(["--config", os.path.join(cdir, f)])))
            e[f]["args"]["config"] = f
    json.dump({"exp-6": e}, open(os.path.join(HERE, "reference_cli_exp6.json"), "w"), indent=1, sort_keys=True)
    print("wrote exp-6 CLI golden:", len(e["defaults"]), "flags,", len(e) - 1, "overlays")


def targets_golden():
    ns = lift(["generate_dynamic_targets_race"], ref=f"{EXP6}/1-main-debias.py")
    rec = {}

    def zip_longest(combs, probs):
        rec["combs"], rec["probs"] = np.array(combs), np.array(probs, dtype=np.float64)
        return itertools.zip_longest(combs, probs)
    ns["ot"] = types.SimpleNamespace(dist=_dist, emd=_emd)
    ns["itertools"] = types.SimpleNamespace(zip_longest=zip_longest)
    out = {}
    for N in NS:
        g = torch.Generator().manual_seed(600 + N)
        nmiss = N // 5 + (1 if N in (3, 16) else 0) + (3 if N == 0 else 0)
        n = N + nmiss
        logits = torch.randn(n, 4, generator=g) * 2.0
        probs = torch.softmax(logits, dim=-1).double()             # fp32 values, carried in float64 (the uncertainties come back uncast)
        miss = torch.randperm(n, generator=g)[:nmiss]
        probs[miss] = -1
        rec.clear()
        t, u = ns["generate_dynamic_targets_race"](probs, w_uncertainty=True)
        assert u.dtype == torch.float64 and int((probs != -1).all(dim=-1).sum()) == N
        out[f"N{N}_combs"] = rec["combs"].reshape(-1, 4).astype(np.int32)
        out[f"N{N}_weights"] = rec["probs"]
        out[f"N{N}_probs"] = probs.numpy()
        out[f"N{N}_targets"] = t.numpy().astype(np.int64)
        out[f"N{N}_uncertainty"] = u.numpy()
    out["Ns"] = np.array(NS, dtype=np.int64)
    path = os.path.join(HERE, "reference_exp6_targets.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes; kept compositions:", {N: len(out[f"N{N}_weights"]) for N in NS})


if __name__ == "__main__":
    if not os.path.isdir(EXP6):
        sys.exit(f"{EXP6} is not available: the exp-6 goldens are generated where the reference tree is mounted")
    cli_golden()
    targets_golden()
