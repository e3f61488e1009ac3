"""Split an HF checkpoint into per-layer safetensors files (reference
``prepare_weights.py``), or write a synthetic random-init model directory.

    python prepare_weights.py <hf_dir> <new_file_dir>
    python prepare_weights.py --synthetic llama2-7b <new_file_dir> [--seed 0] [--dtype bfloat16]
                              [--unique_layers K]   (decoder layers >= K hard-link to layer i % K)
    either form: --quantize fp8 [--fp8_scale channel|tensor|block128]
                 (decoder projection weights as FP8 e4m3 + fp32 scales: half the weight bytes)
                 --quantize int4 [--int4_group 128] [--int4_scale_dtype float16|bfloat16|float32]
                 (the same weights as 4-bit words + group scales, W4A16: a quarter of the bytes)
"""
import argparse
import sys

from flexible_llm_sharding_amd.utils.layer_format import split_into_layers


def main(argv=None):
    ap = argparse.ArgumentParser(description="Split model weights into layers.")
    ap.add_argument("bin_dir", type=str, help="Path to the HF weights directory (or preset name with --synthetic)")
    ap.add_argument("new_file_dir", type=str, help="Path to the new layer-wise file directory")
    ap.add_argument("--synthetic", action="store_true",
                    help="treat bin_dir as a preset name (tiny, small, llama2-7b, llama2-13b, llama2-70b) "
                         "and write random-init weights")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--std", type=float, default=0.02)
    ap.add_argument("--num_hidden_layers", type=int, default=None)
    ap.add_argument("--dtype", choices=["float16", "bfloat16", "float32"], default="float16",
                    help="--synthetic: checkpoint dtype")
    ap.add_argument("--unique_layers", type=int, default=0,
                    help="--synthetic: write K distinct decoder layers, hard-link the rest (disk-limited boxes)")
    ap.add_argument("--quantize", choices=["fp8", "int4"], default=None,
                    help="write the decoder layers' 2-D projection weights (q/k/v/o, gate/up/down, fused and "
                         "expert weights) as FP8 e4m3 with fp32 scales, or as INT4 (W4A16, symmetric) with group "
                         "scales; router, norms, biases, embedding and head stay as they are")
    ap.add_argument("--fp8_scale", choices=["channel", "tensor", "block128"], default="channel",
                    help="--quantize fp8: one scale per output channel / per tensor (weight_scale) or per "
                         "128x128 block (weight_scale_inv)")
    ap.add_argument("--int4_group", type=int, default=128,
                    help="--quantize int4: weights per scale, a multiple of 32 that divides every row length "
                         "(0: one scale per output channel)")
    ap.add_argument("--int4_scale_dtype", choices=["float16", "bfloat16", "float32"], default="float16",
                    help="--quantize int4: dtype of the group scales")
    a = ap.parse_args(argv)
    if a.synthetic:
        import torch
        from flexible_llm_sharding_amd.config import preset
        from flexible_llm_sharding_amd.utils.synthetic import write_synthetic_checkpoint
        kw = {} if a.num_hidden_layers is None else {"num_hidden_layers": a.num_hidden_layers}
        write_synthetic_checkpoint(preset(a.bin_dir, **kw), a.new_file_dir, seed=a.seed, std=a.std,
                                   dtype=getattr(torch, a.dtype), unique_layers=a.unique_layers,
                                   quantize=a.quantize, fp8_scale=a.fp8_scale, int4_group=a.int4_group,
                                   int4_scale_dtype=getattr(torch, a.int4_scale_dtype))
    else:
        import torch
        split_into_layers(a.bin_dir, a.new_file_dir, quantize=a.quantize, fp8_scale=a.fp8_scale,
                          int4_group=a.int4_group, int4_scale_dtype=getattr(torch, a.int4_scale_dtype))
    return 0


if __name__ == "__main__":
    sys.exit(main())
