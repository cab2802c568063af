"""profiles/<tag>_summary.md, <tag>_bench_default.json and traffic.json from gpurun_out/final_<run>/ (the output of
tools/final_profiles.sh): python3 tools/make_summary.py r03 r03"""
import json
import sys

run, tag = sys.argv[1], sys.argv[2]
out = f"gpurun_out/final_{run}/"
d = json.load(open(out + "bench_default.json"))


def table(w):
    lines = open(out + f"summary_{w}.md").read().strip().split("\n")
    return "\n".join(l for l in lines if l.startswith("|") and "torch " not in l and "__amd_rocclr" not in l)


def roofs(x):
    rs = x.get("rooflines", [x["roofline"]])
    return "; ".join(f"{r['symbol']} {r['frac']:.3f} of {r['peak']:g} {r['unit']} ({r['avg_launch_us']:.1f} us"
                     + (f", {r['frac_traffic']:.3f} on PMC bytes" if r.get("frac_traffic") else "") + ")" for r in rs)


def traf(x):
    rs = x.get("rooflines", [x["roofline"]])
    return "; ".join(f"{r['traffic'] / 1e6:.0f} MB" if r.get("traffic") else "-" for r in rs)


o = d["optimizer_step"]
s = f"""# {tag} - rocprofv3 kernel summaries of the three single-GPU bench workloads (end of round 3)

`bash tools/final_profiles.sh {run}` on one MI355X: the `python3 bench.py --full --steps 30 --warmup 5` line is `profiles/{tag}_bench_default.json`; per workload `rocprofv3 --kernel-trace --stats --output-format csv -- python3 bench.py --full --workload W --steps 20 --warmup 3 --no-cpu-baseline --no-graph --no-pmc --no-optimizer` (eager launches so that every kernel is attributed; call counts include the 0.25 s of untimed pre-warm steps; torch's one-off initialisation kernels filtered out; a profiled run holds a 3-5 % lower clock than the un-profiled bench line).

## deepfm

{table('deepfm')}

## xdeepfm

{table('xdeepfm')}

## dcn

{table('dcn')}

## the bench line (profiles/{tag}_bench_default.json)

| workload | examples/s | ms/step | roofline kernels (fraction of the peak named: 8 TB/s HBM, 157.3 TFLOP/s f32 MFMA, 2500 TFLOP/s bf16 MFMA for the split-operand GEMM; avg launch) | PMC traffic per launch | CPU port ex/s ({d['cpu_baseline']['cores']} threads) | optimizer step (reported separately) |
|---|---:|---:|---|---|---:|---:|
| deepfm (configs[1]) | {d['value']:,.0f} | {d['ms_per_step']:.4f} | {roofs(d)} | {traf(d)} | {d['cpu_baseline']['value']:,.0f} | {o['ms']:.4f} ms (sort {o['sort_ms']:.4f} + apply {o['apply_ms']:.4f}; bit-identical rerun: {o['bit_identical_rerun']}) |
| deepfm, Zipf(1.05) ids | {d['zipf']['value']:,.0f} | {d['zipf']['ms_per_step']:.4f} | {roofs(d['zipf'])} | - | - | {(d['zipf'].get('optimizer_step') or {}).get('ms', float('nan')):.4f} ms |
"""
for w in ("xdeepfm", "dcn"):
    x = d["workloads"][w]
    cb = x.get("cpu_baseline", {}).get("value")
    oo = x.get("optimizer_step", {}).get("ms")
    s += (f"| {w} (configs[{2 if w == 'xdeepfm' else 3}]) | {x['value']:,.0f} | {x['ms_per_step']:.4f} | {roofs(x)} | "
          f"{traf(x)} | {cb:,.0f} | {oo:.4f} ms |\n")
sh = d["step_hbm"]
ts = d.get("train_step", {})
s += f"""
Whole DeepFM step on SURVEY 8d's embed+FM bytes: {sh['algorithmic_bytes'] / 1e6:.1f} MB / {d['ms_per_step']:.4f} ms = {sh['achieved']:.0f} GB/s = {sh['frac']:.3f} of spec (0.43 at the end of round 2: 0.1726 ms; the kernel itself moves 362 MB per step on the counters - it is not bandwidth-bound, profiles/r03_deepfm_step.md).

`train_step` (what fit() achieves at configs[1]: new batch -> fwd+bwd -> row-wise lazy Adam, sort on a side stream -> dense Adam): {ts.get('ms_per_step_dataset_in_hbm')} ms per step with the dataset in HBM, {ts.get('ms_per_step_pinned_feeder')} ms through the zero-copy pinned feeder (PCIe floor {ts.get('pcie_floor_ms_at_63GBs')} ms for the int64 ids).

Round 2 -> round 3 on the same command: DeepFM 380 M -> {d['value'] / 1e6:.0f} M examples/s (the whole training step as ONE kernel, rm_deepfm_step: profiles/r03_deepfm_step.md); optimizer step 0.39 -> {o['ms']:.2f} ms (field-segmented sort 152 -> 62 us, long runs in segments: Zipf 0.66 -> 0.34 ms; profiles/r03_optimizer.md); DCN 45.7 M -> {d['workloads']['dcn']['value'] / 1e6:.1f} M (all six dense GEMMs on the bf16 matrix pipe with split fp32 operands, rm_dense_fwd6 / rm_dense_wgrad6: profiles/r03_dense_bf16x6.md); xDeepFM 4.33 M -> {d['workloads']['xdeepfm']['value'] / 1e6:.2f} M (CIN's second layer - forward, dX, dW - on the same scheme, csrc/cin6.hip); configs[4] through the sharded engine at world size 1, per-GPU batch 8192: 7.96 -> {d['workloads']['xdeepfm_100m']['ms_per_step']:.2f} ms; the row-sharded DeepFM step at world size 1 0.366 -> 0.25 ms (profiles/r03_sharded_step.md).
"""
open(f"profiles/{tag}_summary.md", "w").write(s)
json.dump(d, open(f"profiles/{tag}_bench_default.json", "w"), indent=1)
src = (f"profiles/{tag}_bench_default.json (rocprofv3 --pmc FETCH_SIZE x2 + WRITE_SIZE child passes of the round-3 "
       "default bench run)")
t = {"deepfm": {}, "xdeepfm": {}, "dcn": {}}
for r in d.get("rooflines", [d["roofline"]]):
    if r.get("traffic"):
        t["deepfm"][r["symbol"]] = {"bytes": r["traffic"], "source": src}
for w in ("xdeepfm", "dcn"):
    x = d["workloads"][w]
    for r in x.get("rooflines", [x["roofline"]]):
        if r.get("traffic"):
            t[w][r["symbol"]] = {"bytes": r["traffic"], "source": src}
json.dump(t, open("profiles/traffic.json", "w"), indent=1)
print("written")
