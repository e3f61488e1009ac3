"""Split an HF checkpoint into per-layer safetensors files (reference
``prepare_weights.py``), or write a synthetic random-init model directory.

    python prepare_weights.py <hf_dir> <new_file_dir>
    python prepare_weights.py --synthetic llama2-7b <new_file_dir> [--seed 0] [--dtype bfloat16]
                              [--unique_layers K]   (decoder layers >= K hard-link to layer i % K)
    either form: --quantize fp8 [--fp8_scale channel|tensor|block128]
                 (decoder projection weights as FP8 e4m3 + fp32 scales: half the weight bytes)
                 --quantize int4 [--int4_group 128] [--int4_scale_dtype float16|bfloat16|float32]
                 (the same weights as 4-bit words + group scales, W4A16: a quarter of the bytes)
                 --quantize nf4 [--nf4_block 64] [--nf4_double_quant true|false]
                 (the same weights in the bitsandbytes 4-bit form, NF4 code book: the QLoRA base)
    python prepare_weights.py <model_dir> <new_file_dir> --merge_lora <adapter_dir> [--lora_scale 1.0]
                 (the fp16 checkpoint with a LoRA adapter merged in: what --lora computes in HBM)
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
    ap.add_argument("--quantize", choices=["fp8", "int4", "nf4"], default=None,
                    help="write the decoder layers' 2-D projection weights (q/k/v/o, gate/up/down, fused and "
                         "expert weights) as FP8 e4m3 with fp32 scales, as INT4 (W4A16, symmetric) with group "
                         "scales, or as bitsandbytes 4-bit (NF4 code book, block absmax); router, norms, biases, embedding and head stay as they are")
    ap.add_argument("--fp8_scale", choices=["channel", "tensor", "block128"], default="channel",
                    help="--quantize fp8: one scale per output channel / per tensor (weight_scale) or per "
                         "128x128 block (weight_scale_inv)")
    ap.add_argument("--int4_group", type=int, default=128,
                    help="--quantize int4: weights per scale, a multiple of 32 that divides every row length "
                         "(0: one scale per output channel)")
    ap.add_argument("--int4_scale_dtype", choices=["float16", "bfloat16", "float32"], default="float16",
                    help="--quantize int4: dtype of the group scales")
    ap.add_argument("--nf4_block", type=int, default=64,
                    help="--quantize nf4: weights per absmax block, a multiple of 32 that divides every tensor's size")
    ap.add_argument("--nf4_double_quant", choices=["true", "false"], default="true",
                    help="--quantize nf4: store the absmax values 8-bit quantised in nested blocks of 256")
    ap.add_argument("--merge_lora", type=str, default=None, metavar="DIR",
                    help="write bin_dir (per-layer files or an HF directory of safetensors files, fp16 / bf16 / "
                         "fp32) with the LoRA adapter DIR merged into its weights, as fp16: the twin of a run with "
                         "--lora DIR.  Runs on the GPU when there is one; otherwise by the numpy definition, layer "
                         "by layer, which is slow for large models")
    ap.add_argument("--lora_scale", type=float, default=None, help="--merge_lora: multiplies alpha / r (default 1.0)")
    a = ap.parse_args(argv)
    if a.lora_scale is not None and not a.merge_lora:
        ap.error("--lora_scale needs --merge_lora")
    if a.merge_lora:
        if a.quantize:
            ap.error("--quantize does not combine with --merge_lora (the merged weights are fp16; quantise them "
                     "in a second step)")
        if a.synthetic:
            ap.error("--synthetic does not combine with --merge_lora (write the checkpoint first)")
        import torch
        from flexible_llm_sharding_amd import lora
        from flexible_llm_sharding_amd.config import ModelConfig
        adapter = lora.LoraAdapter.load(ModelConfig.from_pretrained(a.bin_dir), a.merge_lora,
                                        1.0 if a.lora_scale is None else a.lora_scale)
        device = torch.device("cuda", 0) if torch.cuda.is_available() else torch.device("cpu")
        lora.write_twin(a.bin_dir, adapter, a.new_file_dir, merge=lora.ops_merge(device))
        return 0
    if a.synthetic:
        import torch
        from flexible_llm_sharding_amd.config import preset
        from flexible_llm_sharding_amd.utils.synthetic import write_synthetic_checkpoint
        kw = {} if a.num_hidden_layers is None else {"num_hidden_layers": a.num_hidden_layers}
        write_synthetic_checkpoint(preset(a.bin_dir, **kw), a.new_file_dir, seed=a.seed, std=a.std,
                                   dtype=getattr(torch, a.dtype), unique_layers=a.unique_layers,
                                   quantize=a.quantize, fp8_scale=a.fp8_scale, int4_group=a.int4_group,
                                   int4_scale_dtype=getattr(torch, a.int4_scale_dtype), nf4_block=a.nf4_block,
                                   nf4_double_quant=a.nf4_double_quant == "true")
    else:
        import torch
        split_into_layers(a.bin_dir, a.new_file_dir, quantize=a.quantize, fp8_scale=a.fp8_scale,
                          int4_group=a.int4_group, int4_scale_dtype=getattr(torch, a.int4_scale_dtype),
                          nf4_block=a.nf4_block, nf4_double_quant=a.nf4_double_quant == "true")
    return 0


if __name__ == "__main__":
    sys.exit(main())
