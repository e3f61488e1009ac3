"""What v_cvt_scalef32_pk_f16_fp4 computes on this GPU, against the MXFP4 definition (mxfp4.dequantize).

For every scale byte e in 0..255 (operand: the fp32 with bits e << 23), every byte select 0..3 and
every nibble u, a source dword holds u in the low nibble and 15 - u in the high nibble of the selected
byte and zeros elsewhere.  The low half of the result is compared with the definition's value of
(u, e), the high half with that of (15 - u, e).  Prints, per byte select and half, the ranges of e in
which any nibble differs, and writes the whole table as JSON.

    python scripts/mxfp4_probe.py [--lib libmxfp4_probe.so] [--out table.json]

Without --lib the probe kernel is compiled with hipcc into a temporary directory, removed afterwards;
``--build_only DIR`` compiles it into DIR ahead of time, for ``--lib DIR/libmxfp4_probe.so``.  The scale
bytes at which anything differs are the ones ``dequant_mxfp4_kernel`` (``csrc/kernels/dequant.hip``)
must not give to the instruction: as measured, e = 255 alone.
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from flexible_llm_sharding_amd import mxfp4  # noqa: E402

SOURCE = r"""
#include <hip/hip_runtime.h>
#include <cstdint>
typedef _Float16 half2_t __attribute__((ext_vector_type(2)));
template <int SEL> __device__ uint32_t cvt(uint32_t w, float sc) {
  return __builtin_bit_cast(uint32_t, (half2_t)__builtin_amdgcn_cvt_scalef32_pk_f16_fp4(w, sc, SEL));
}
// 256 blocks (e) of 64 threads (sel * 16 + u); out[(e * 4 + sel) * 16 + u], 16384 dwords
__global__ void probe_kernel(uint32_t* out) {
  const uint32_t e = blockIdx.x, u = threadIdx.x & 15u, sel = (threadIdx.x >> 4) & 3u;
  const uint32_t w = (u | ((15u - u) << 4)) << (8u * sel);
  const float sc = __uint_as_float(e << 23);
  const uint32_t r = sel == 0 ? cvt<0>(w, sc) : sel == 1 ? cvt<1>(w, sc) : sel == 2 ? cvt<2>(w, sc) : cvt<3>(w, sc);
  out[(e * 4u + sel) * 16u + u] = r;
}
extern "C" int mxfp4_probe(uint32_t* out) {
  hipLaunchKernelGGL(probe_kernel, dim3(256), dim3(64), 0, 0, out);
  return (int)hipDeviceSynchronize();
}
"""


def build(out_dir: str) -> str:
    src, lib = os.path.join(out_dir, "mxfp4_probe.hip"), os.path.join(out_dir, "libmxfp4_probe.so")
    with open(src, "w") as f:
        f.write(SOURCE)
    hipcc = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O2", "-fPIC", "-shared", "-Xclang", "-target-feature", "-Xclang",
                    "-packed-fp32-ops", src, "-o", lib], check=True)
    return lib


def ranges(es):
    """[[lo, hi], ...] of the sorted integers ``es``."""
    out = []
    for e in es:
        if out and out[-1][1] == e - 1:
            out[-1][1] = e
        else:
            out.append([e, e])
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=None, help="path of a probe library compiled before with --build_only")
    ap.add_argument("--build_only", default=None, metavar="DIR", help="compile the probe into DIR and stop")
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    if a.build_only:
        print(build(a.build_only))
        return 0
    if not torch.cuda.is_available():
        raise SystemExit("mxfp4_probe needs the GPU: the table is a measurement")
    if a.lib:
        lib = ctypes.CDLL(a.lib)
    else:
        with tempfile.TemporaryDirectory() as tmp:      # (the loaded library outlives its file)
            lib = ctypes.CDLL(build(tmp))
    lib.mxfp4_probe.restype, lib.mxfp4_probe.argtypes = ctypes.c_int, [ctypes.c_void_p]
    out = torch.zeros(256 * 4 * 16, dtype=torch.int32, device="cuda")
    rc = lib.mxfp4_probe(out.data_ptr())
    if rc:
        raise SystemExit(f"probe failed: hip error {rc}")
    got = out.cpu().numpy().view(np.uint32).reshape(256, 4, 16)
    u = torch.arange(16, dtype=torch.uint8).repeat(256, 2)
    want = mxfp4.dequantize(mxfp4.pack(u), torch.arange(256).to(torch.uint8).reshape(256, 1), (256, 32))
    want = want.view(torch.int16).numpy().view(np.uint16)[:, :16].astype(np.uint32)          # [e, u]
    lo_ok = (got & 0xFFFF) == want[:, None, :]
    hi_ok = (got >> 16) == want[:, None, ::-1]
    report = {"differs": {}, "hardware": got.tolist(), "definition": want.tolist()}
    for sel in range(4):
        for half, ok in (("low", lo_ok), ("high", hi_ok)):
            report["differs"][f"sel{sel}_{half}"] = ranges([e for e in range(256) if not ok[e, sel].all()])
    same = [e for e in range(256) if lo_ok[e].all() and hi_ok[e].all()]
    report["equal"] = ranges(same)
    print("e ranges where the instruction equals the definition for all nibbles, selects and halves:", report["equal"])
    for k, v in report["differs"].items():
        print(f"  {k}: differs for e in {v}")
    for e in (0, 1, 102, 103, 104, 113, 141, 142, 254, 255):
        print(f"  e={e}: hardware {[hex(int(x) & 0xFFFF) for x in got[e, 0]]}\n         definition {[hex(int(x)) for x in want[e]]}")
    if a.out:
        with open(a.out, "w") as f:
            json.dump(report, f)
    return 0


if __name__ == "__main__":
    sys.exit(main())
