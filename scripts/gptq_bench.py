"""Time of the GPTQ / AWQ repack (step A, fls_repack_w4) and of the expansion with zero points (step B,
fls_dequant_w4z) against the INT4 chain on the same N and g (profiles/gptq/README.md).  Figures only,
nothing pass/fail.

  python scripts/gptq_bench.py [--iters N] [--rounds R] [--group 128] [--shapes 8192x28672,8192x8192]
        # in one process, per shape R rounds alternating five cases in place on an out x in tensor: step A for
        # both layouts, step B, both steps as the loader enqueues them (GPTQ), and fls_dequant_int4 (fp16
        # scales).  Per round and case: median and minimum of N timed calls after 3 warm-up calls (device
        # events around each call; the bytes the case reads are restored outside them) and GB/s of the bytes
        # the case reads plus writes.  Then the medians over the rounds and (A + B) / INT4.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _time(fn, prep, iters):
    times = []
    for i in range(iters + 3):
        prep()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        if i >= 3:
            times.append(e0.elapsed_time(e1) * 1e-3)
    return float(np.median(times)), min(times)


def bench(out: int, inn: int, g: int, iters: int, rounds: int) -> dict:
    from flexible_llm_sharding_amd import _native, gptq, int4
    from flexible_llm_sharding_amd.ops import get_ops
    from flexible_llm_sharding_amd.ops.hip_backend import _chk, _stream
    dev = torch.device("cuda", 0)
    ops, k = get_ops(dev), _native.kernels()
    n, G = out * inn, inn // g
    region = torch.empty(2 * n, dtype=torch.uint8, device=dev)
    (q0, qn), (s0, sn), (z0, zn) = gptq.input_layout(out, inn, g)
    top = gptq.region_layout(n, g)[0].scale_off
    # the landed file tensors: random words and zero points, scales about 1e-3 (the layouts share the byte counts)
    bottom = torch.randint(0, 256, (z0 + zn,), dtype=torch.uint8, device=dev)
    bottom[s0:s0 + sn] = ((torch.rand(G * out, device=dev) + 0.5) * 1e-3).to(torch.float16).view(torch.uint8)
    p = region.data_ptr()

    def step_a(code):
        return lambda: _chk(k.fls_repack_w4(p, out, inn, g, code, _stream()), "fls_repack_w4")

    region[:z0 + zn].copy_(bottom)
    step_a(0)()
    torch.cuda.synchronize()
    repacked = region[top:].clone()                     # what step B reads
    ibase, ispan = int4.landing_span(n, g, 2)
    int4.land(region, torch.randint(0, 256, (n // 2,), dtype=torch.uint8, device=dev), bottom[s0:s0 + sn], n, g, 2)
    landed4 = region[ibase:].clone()
    in_a, out_a = z0 + zn, n // 2 + 4 * n // g

    def put_bottom():
        region[:z0 + zn].copy_(bottom)

    cases = {
        "repack_gptq": (step_a(0), put_bottom, in_a + out_a),
        "repack_awq": (step_a(1), put_bottom, in_a + out_a),
        "dequant_w4z": (lambda: _chk(k.fls_dequant_w4z(p, n, g, _stream()), "fls_dequant_w4z"),
                        lambda: region[top:].copy_(repacked), out_a + 2 * n),
        "gptq_both": (lambda: ops.dequant_gptq(region, out, inn, g, "gptq"), put_bottom, in_a + 2 * out_a + 2 * n),
        "dequant_int4": (lambda: ops.dequant_int4(region, n, g, torch.float16), lambda: region[ibase:].copy_(landed4),
                         n // 2 + 2 * n // g + 2 * n),
    }
    meds = {name: [] for name in cases}
    for rnd in range(rounds):
        for name, (fn, prep, moved) in cases.items():
            med, mn = _time(fn, prep, iters)
            meds[name].append(med)
            print(json.dumps({"case": name, "round": rnd, "shape": [out, inn], "group": g, "median_us": med * 1e6,
                              "min_us": mn * 1e6, "read_plus_written_GB_per_s_median": moved / med / 1e9,
                              "iters": iters}), flush=True)
    res = {name: {"median_us": float(np.median(v)) * 1e6, "spread_pct": (max(v) - min(v)) / float(np.median(v)) * 100,
                  "read_plus_written_GB_per_s": cases[name][2] / float(np.median(v)) / 1e9} for name, v in meds.items()}
    t = {name: float(np.median(v)) for name, v in meds.items()}
    res.update(shape=[out, inn], group=g, launches_w4z=int(k.fls_dequant_w4z_launches(n, g)),
               launches_int4=int(k.fls_dequant_int4_launches(n, g, 2)),
               gptq_a_plus_b_over_int4=(t["repack_gptq"] + t["dequant_w4z"]) / t["dequant_int4"],
               awq_a_plus_b_over_int4=(t["repack_awq"] + t["dequant_w4z"]) / t["dequant_int4"],
               gptq_both_over_int4=t["gptq_both"] / t["dequant_int4"])
    return res


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--group", type=int, default=128)
    ap.add_argument("--shapes", default="8192x28672,8192x8192")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("gptq_bench needs the GPU")
    for sh in a.shapes.split(","):
        out, inn = (int(x) for x in sh.split("x"))
        print(json.dumps(bench(out, inn, a.group, a.iters, a.rounds)), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
