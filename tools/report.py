#!/usr/bin/env python3
"""Runs bench.py over every BASELINE.json configuration that fits one GPU (and the per-rank slice of
the EP=8 one), uniform and Zipf routing, and writes a markdown table + the raw JSON lines.
  python tools/report.py [out_dir]          (on the GPU box)
"""
import json
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
OUT = Path(sys.argv[1]) if len(sys.argv) > 1 else ROOT / "gpurun_out"
# optional second argument: comma list of workload names -- re-measure only those rows and merge them into the
# report.md / report.jsonl already in OUT
ONLY = set(sys.argv[2].split(",")) if len(sys.argv) > 2 else None
RUNS = [
    ("1 Qwen3-30B-A3B bf16 M=1", "qwen3_30b_a3b_bf16_decode_m1", 300, 2.5e3, 2.0),
    ("2 Mixtral-8x7B bf16 M=32", "mixtral8x7b_bf16_decode_m32", 200, 2.5e3, 2.0),
    ("2b Mixtral-8x7B fp8-W8A8 M=32", "mixtral8x7b_fp8w8a8_decode_m32", 200, 2.5e3, 1.0),
    ("3 Mixtral-8x7B int4-g128 M=128", "mixtral8x7b_int4g128_decode_m128", 200, 2.5e3, 0.5),
    ("3' same, int4 fast mode (opt-in)", "mixtral8x7b_int4g128_fast_decode_m128", 200, 2.5e3, 0.5),
    ("3'' same, uint4 with zero points (AWQ-style, LKM_INT4_ZP)", "mixtral8x7b_int4g128_zp_decode_m128", 200, 2.5e3, 0.5),
    ("3b Mixtral-8x7B MXFP4 M=128", "mixtral8x7b_mxfp4_decode_m128", 200, 2.5e3, 0.5),
    ("3c Mixtral-8x7B NVFP4 M=128", "mixtral8x7b_nvfp4_decode_m128", 200, 2.5e3, 0.5),
    ("3d Mixtral-8x7B MXFP4 M=32", "mixtral8x7b_mxfp4_decode_m32", 200, 2.5e3, 0.5),
    ("4 DSv3-style fp8-W8A8, EP=8 rank slice (32 experts, 256 rows)", "dsv3_ep8_rank_fp8w8a8_rows256", 200, 2.5e3, 1.0),
    ("4b same, fp8-W8A16 (lk_moe semantics)", "dsv3_ep8_rank_fp8w8a16_rows256", 200, 2.5e3, 1.0),
    ("4c DSv3-style fp8-W8A8, all 256 experts on one GPU, M=256, grouped sigmoid router", "dsv3_fp8w8a8_ep_decode_b256", 100, 2.5e3, 1.0),
    ("5 GLM-4.5-Air prefill M=8192 (bf16 weights)", "glm45air_bf16_prefill_m8192", 20, 2.5e3, 2.0),
    ("5b GLM-4.5-Air prefill M=8192 (fp8-W8A8)", "glm45air_fp8w8a8_prefill_m8192", 20, 2.5e3, 1.0),
    ("5c GLM-4.5-Air prefill M=8192 (fp8-W8A16, MOE_FP8.gpu_prefill)", "glm45air_fp8w8a16_prefill_m8192", 20, 2.5e3, 1.0),
    ("5d Mixtral-8x7B int4-g128 prefill M=4096 (MOE_WNA16.gpu_prefill)", "mixtral8x7b_int4g128_prefill_m4096", 20, 2.5e3, 0.5),
]


def run(workload, steps, routing):
    cmd = [sys.executable, str(ROOT / "bench.py"), "--workload", workload, "--steps", str(steps), "--warmup",
           "5", "--full", "--no-cpu-baseline", "--no-extras", "--full-line", "--routing", routing]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    for line in r.stdout.splitlines():
        if line.startswith("{"):
            return json.loads(line)
    raise RuntimeError(f"{workload}: no JSON line\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")


def main():
    OUT.mkdir(parents=True, exist_ok=True)
    rows, raw = [], []
    for name, wl, steps, mfma_peak, _ in RUNS:
        if ONLY is not None and wl not in ONLY:
            continue
        # (the sigmoid + bias routers also under the synthetic N(0, 0.1) score-correction bias of rounds 1-5: a skewed routing,
        # labelled "biased"; their "uniform" and "zipf" rows run a zero bias)
        biased = wl.startswith("glm45air") or wl == "dsv3_fp8w8a8_ep_decode_b256"
        for routing in ("uniform", "zipf") + (("biased",) if biased else ()):
            try:
                j = run(wl, steps, routing)
            except Exception as e:  # keep going: one failing config must not hide the others
                rows.append(f"| {name} | {routing} | FAILED: {str(e)[:80]} |")
                continue
            raw.append(j)
            rf, lay, km = j["roofline"], j["roofline"]["layer"], j["roofline"]["kernel_ms"]
            stp = rf.get("step", {})
            # the same columns as the bench line's `roofline` (bench.py roof_fields): the dominant kernel against both peaks
            # and against roof = min(MFMA peak, AI x HBM peak), then the whole step against the same two peaks
            rows.append(
                f"| {name} | {routing} | {j['ms_per_step']*1e3:.1f} | {j['value']:.0f} | {lay['routed_rows']} / {lay['experts_hit']} | "
                f"{km['sort']*1e3:.1f} / {km['gemm1']*1e3:.1f} / {km['gemm2']*1e3:.1f} / {km['combine']*1e3:.1f} | "
                f"{rf['GBps']:.0f} ({rf['hbm_frac']*100:.1f} %) | {rf['tflops']:.1f} ({rf['mfma_frac']*100:.2f} % of {rf['mfma_peak_tflops']/1e3:.1f} PF) | "
                f"{rf['roof_tflops']:.0f} ({rf['roof_bound']}) | {rf['frac_of_roof']:.3f} | "
                f"{lay['GBps_over_step']:.0f} ({stp.get('hbm_frac', 0)*100:.1f} %) | {lay['TFLOPs_over_step']:.1f} ({stp.get('mfma_frac', 0)*100:.2f} %) | "
                f"{stp.get('frac_of_roof', 0):.3f} | {j['config']['geometry'].split('|',2)[2].strip()} |")
    hdr = ("| config | routing | step µs (graph, incl. router) | tokens/s | routed rows / experts hit | "
           "kernel µs sort / gemm1 / gemm2 / combine (HIP events) | GEMM1 GB/s (hbm_frac of 8 TB/s) | GEMM1 TFLOP/s (mfma_frac of the dense peak) | "
           "roof TFLOP/s = min(MFMA, AI x HBM) (bound) | GEMM1 frac_of_roof | step: weight GB/s (hbm_frac) | step: TFLOP/s (mfma_frac) | "
           "step frac_of_roof | geometry |\n|---|---|---|---|---|---|---|---|---|---|---|---|---|---|")
    if ONLY is not None and (OUT / "report.md").exists():
        key = lambda line: tuple(c.strip() for c in line.split("|")[1:3])
        fresh = {key(r): r for r in rows}
        rows = [fresh.pop(key(l), l) for l in (OUT / "report.md").read_text().splitlines()[2:] if l.strip()]
        rows += list(fresh.values())
        old = [json.loads(l) for l in (OUT / "report.jsonl").read_text().splitlines() if l.strip()]
        jkey = lambda j: (j["config"]["workload"], j["config"]["routing"])
        new = {jkey(j): j for j in raw}
        raw = [new.pop(jkey(j), j) for j in old] + list(new.values())
    md = hdr + "\n" + "\n".join(rows) + "\n"
    (OUT / "report.md").write_text(md)
    (OUT / "report.jsonl").write_text("\n".join(json.dumps(x) for x in raw) + "\n")
    print(md)


if __name__ == "__main__":
    main()
