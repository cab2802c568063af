"""What the tools/bench_*.py share: the timing loop, the batch of the engine steps, the HBM fields of a kernel record
and the command line.  Each tool keeps its kernels, its comparator and its shapes; iteration counts that differ from
the defaults are passed where they are used (the numbers under profiles/ were taken with them)."""
import json
import sys

import torch

from recman_amd import engine as eng

PEAK_HBM, PEAK_MFMA = 8.0e12, 157.3e12   # bytes/s (the HBM spec), flop/s (dense f32 MFMA)


def stats(ts):
    ts = sorted(ts)
    return dict(min=round(ts[0], 4), median=round(ts[len(ts) // 2], 4), mean=round(sum(ts) / len(ts), 4))


def times(fns, n, warm, indexed=False):
    """The ms of every timed launch per contender (hipEvent pairs), the contenders taking turns, after `warm`
    untimed rounds (clocks and caches).  indexed: fn(i) gets the round's number (to rotate through buffer sets)."""
    for i in range(warm):
        for fn in fns:
            fn(i) if indexed else fn()
    ts = [[] for _ in fns]
    for i in range(n):
        for fn, acc in zip(fns, ts):
            a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn(i) if indexed else fn()
            z.record()
            z.synchronize()
            acc.append(a.elapsed_time(z))
    return ts


def alternate(fns, n=50, warm=5, indexed=False):
    """min / median / mean ms per contender (stats), the contenders taking turns (times)."""
    return [stats(t) for t in times(fns, n, warm, indexed)]


def medians(fns, n, warm):
    """The unrounded median ms per contender (times): the older tools round what they derive from it."""
    return [sorted(t)[len(t) // 2] for t in times(fns, n, warm)]


def hashed_batch(B=65536, F=26, Dn=13, rows=40000):
    """(spec, idx, dense, g): hashed ids over F x `rows` table rows and Dn normal dense columns on the GPU, drawn
    from the CPU generator g (seed 0), which the caller draws its labels from."""
    g = torch.Generator().manual_seed(0)
    sizes = [rows] * F
    idx = torch.stack([torch.randint(0, v, (B,), generator=g) for v in sizes], 1).cuda()
    dense = torch.randn(B, Dn, generator=g).cuda()
    spec = eng.FeatureSpec([f"C{i}" for i in range(F)], sizes, [f"I{j}" for j in range(Dn)])
    return spec, idx, dense, g


def criteo_like(B=65536, F=26, Dn=13):
    """(spec, idx, dense, y): hashed_batch with 0/1 labels, about 30 % ones."""
    spec, idx, dense, g = hashed_batch(B, F, Dn)
    return spec, idx, dense, (torch.rand(B, generator=g) < 0.3).long().cuda()


def hbm_fields(fwd_bytes, bwd_bytes, fwd, bwd, peak_share=True):
    """A kernel pair's algorithmic bytes against its median times (stats): {fwd,bwd}_hbm_gb, _hbm_tb_s and - unless
    the record prices the pair on another roofline - _peak_share of the 8 TB/s HBM spec."""
    work = dict(fwd=(fwd_bytes, fwd["median"] * 1e-3), bwd=(bwd_bytes, bwd["median"] * 1e-3))
    rec = {f"{k}_hbm_gb": round(b / 1e9, 4) for k, (b, _) in work.items()}
    rec.update({f"{k}_hbm_tb_s": round(b / s / 1e12, 3) for k, (b, s) in work.items()})
    if peak_share:
        rec.update({f"{k}_peak_share": round(b / s / PEAK_HBM, 4) for k, (b, s) in work.items()})
    return rec


def hbm_gb_s_fields(fwd_bytes, bwd_bytes, fwd, bwd, share):
    """The same in GB/s: {fwd,bwd}_hbm_gb, _gb_s and _{share}, the rounded rate's share of the HBM spec."""
    work = dict(fwd=(fwd_bytes, fwd["median"] * 1e-3), bwd=(bwd_bytes, bwd["median"] * 1e-3))
    rec = {f"{k}_hbm_gb": round(b / 1e9, 4) for k, (b, _) in work.items()}
    rec.update({f"{k}_gb_s": round(b / s / 1e9, 1) for k, (b, s) in work.items()})
    rec.update({f"{k}_{share}": round(rec[f"{k}_gb_s"] * 1e9 / PEAK_HBM, 4) for k in work})
    return rec


def selected(kernels, steps):
    """{"kernels": kernels(comparator), "steps": steps()}: `--kernels-only` launches nothing but the fused kernels
    (no comparator, no step), `--step-only` nothing but the engine's step - the runs to put under a kernel trace."""
    only, step_only = "--kernels-only" in sys.argv, "--step-only" in sys.argv
    res = {}
    if not step_only:
        res["kernels"] = kernels(not only)
    if not only:
        res["steps"] = steps()
    return res


def emit(res):
    """One JSON line per kernel record, one for the steps, one per further key; `--json FILE` keeps all of res."""
    for k in res.get("kernels", ()):
        print(json.dumps(k), flush=True)
    if "steps" in res:
        print(json.dumps(res["steps"]), flush=True)
    for k in res:
        if k not in ("kernels", "steps"):
            print(json.dumps({k: res[k]}), flush=True)
    if "--json" in sys.argv:
        with open(sys.argv[sys.argv.index("--json") + 1], "w") as f:
            json.dump(res, f, indent=1)


def main(kernels, steps):
    emit(selected(kernels, steps))
