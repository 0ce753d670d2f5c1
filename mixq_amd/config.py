"""Per-model switches of the MI355X operator, captured at construction.

Rounds 1-4 kept these as seven process-global module variables (`linear.PACK_FMT`, `fused.JOINT_GATE_UP`, ...): two models in one process
changed each other's kernels and cache keys.  Now a `MixqConfig` lives on the model's `MixLibCache` (`cache.config`; the reference builds
ONE cache per model and hands it to every layer, mixquant/Cache.py:5, models/llama.py) and every layer / fused module keeps a reference to
the config of the cache it was built with - a layer built without a cache gets its own.  The reference has no counterpart: its only
switches are constructor arguments of the same objects."""
from __future__ import annotations

from dataclasses import dataclass, replace

import torch

from ._capi import FMT_F16X64, FMT_F6X128


@dataclass
class MixqConfig:
    # Packed layout 8-bit layers keep their weights in (and ask their activations in): MIXQ_FMT_F16X64 feeds the weights-in-registers GEMM
    # of gemm_wreg.hip, MIXQ_FMT_P16X64 the LDS-staged one of gemm.hip (include/mixq_hip.h).
    pack_fmt: int = FMT_F16X64
    # ... and 4-bit layers: MIXQ_FMT_F6X128 - both operands as FP6 E3M2 codes, the W4A4 GEMM on the FP6 matrix pipe (gfx950 has no int4
    # MFMA; every integer of [-8, 8] is an E3M2 value and the fp32 accumulator is exact, so the result is the int4 contraction bit for bit
    # at 1.6x the int8 MFMA rate).  FMT_P16X64 selects the int8-expansion kernel instead (nibbles, two thirds of the FP6 image's bytes).
    pack_fmt4: int = FMT_F6X128
    # ONE resident weight image per 4-bit layer: the FP6 one (0.75 byte per weight).  A decode-heavy deployment of NARROW layers may opt
    # into a SECOND, nibble image for batches of at most this many rows (32 is the useful value; profiles/r04_w4a4_small_batch.txt).  0 = off.
    small_batch_m4: int = 0
    # After a layer's outlier search has frozen, keep ONLY the packed weight image in HBM (the plain [N,K] `q_weight` is re-created on
    # demand for state_dict / attribute reads).  False keeps both copies (2x the reference's weight memory).
    compact_weights: bool = True
    # Frozen layers run their forward (extract + quantise, GEMM) through ONE C-ABI call on a kept argument block (mixq_linear_forward).
    # False keeps the two-call route (same kernels, same results; the parity tests compare the two).
    one_call_forward: bool = True
    # gate_proj's GEMM also emits down_proj's per-row |x| maxima (mixq_gemm_i8_fused_amax); False = the two-pass quantiser
    fuse_down_amax: bool = True
    # gate_proj + up_proj of MixLlamaMLP as one launch over an interleaved weight image once both predictions are frozen; False = up_proj's
    # launch, then gate_proj's with the SiLU-and-multiply epilogue
    joint_gate_up: bool = True
    # the fused norm hands the next (frozen) layer's kept outlier map to its quantise step (mixq_rmsnorm_quant_fused_masked); False = the
    # column mask is built inside the kernel on every launch
    norm_kept_map: bool = True
    # The model's activation dtype: ONE per model.  A layer takes x of exactly this dtype and returns y in it (torch.float16, the
    # reference's, or torch.bfloat16: DESIGN.md section 2).  x_scale, scale_col, bias, sigma and the weight_cache buffer are float16 in
    # either case; y, x_out / activation_outliers and an addend / multiplier follow this switch.  Served in bfloat16: MixLinear_GEMM
    # (W8A8 and W4A4) and, behind `fused_bf16` below, FasterTransformerRMSNorm and MixLlamaMLP (its joint gate / up launch behind
    # `joint_gate_up_bf16` on top of that) and, behind `w8a16_bf16`, weight_only (W8A16) layers.
    act_dtype: torch.dtype = torch.float16
    # Opt-in to the bfloat16 forms of the fused modules (fused.py): with act_dtype=torch.bfloat16 and fused_bf16=True,
    # FasterTransformerRMSNorm runs the bf16 norm + extract + quantise pass (mixq_rmsnorm*_bf16) and MixLlamaMLP the two-launch route with the
    # SiLU-and-multiply epilogue and the row-maximum hand-over to down_proj.  The default is off ONLY because the refusal of these modules
    # under a bfloat16 config (NotImplementedError at construction) is pinned behaviour of this ABI minor; nothing else speaks against it.
    # Without act_dtype=torch.bfloat16 the switch does nothing.  Not part of key(): it selects no GEMM plan and no weight image.
    fused_bf16: bool = False
    # Opt-in to the joint gate / up launch of a bfloat16 MixLlamaMLP (mixq_gemm_i8_pair_bf16 / mixq_gemm_i4_pair_bf16, ABI 1.5): the same
    # bytes as the two-launch route from one launch.  It has an effect only with act_dtype=torch.bfloat16, fused_bf16=True and
    # joint_gate_up=True.  The default is off ONLY because the refusal is pinned behaviour (a bfloat16 block's `_joint_applies` answers False
    # under the default flags); nothing else speaks against it.  Not part of key(): the joint image's identity already carries act_dtype,
    # and the switch selects a route, not an image.
    joint_gate_up_bf16: bool = False
    # Opt-in to bfloat16 weight-only (W8A16) layers (mixq_gemm_w8a16_bf16, ABI 1.6): with act_dtype=torch.bfloat16 and w8a16_bf16=True a
    # MixLinear_GEMM(weight_only=True) is built and runs on bf16 x - GPT-J's fc_out, MixGPTJMLP, `extra_weight_only=` layers.  The default is
    # off ONLY because the ValueError for such a layer under a bfloat16 config is pinned behaviour; nothing else speaks against it.  Without
    # act_dtype=torch.bfloat16 the switch does nothing.  Not part of key(): it selects no GEMM plan and no joint image.
    w8a16_bf16: bool = False
    # Opt-in to the small-batch ("decode") kernel in bfloat16 (mixq_gemm_i8_decode_bf16 / mixq_gemm_i4_decode_bf16, ABI 1.7): with
    # act_dtype=torch.bfloat16 and decode_bf16=True a MixLinear_GEMM takes, at M <= 32, the route fp16 takes there - N / 32 workgroups x 8
    # k-split waves instead of the 32 x 64 tiling's N / 64 workgroups - wherever mixq_gemm_decode_pick_bf16 answers 1 and no row maximum is
    # asked of the GEMM; a 4-bit layer under small_batch_m4 > 0 then serves those batches from its nibble image.  The default is off because
    # the route of a bf16 layer at small batch is observable behaviour of this ABI minor: with outlier columns the two routes differ in the
    # tail's summation order, hence in bytes.  Without act_dtype=torch.bfloat16 the switch does nothing.  Not part of key(): it selects a route
    # over images that already exist (a kept plan's identity carries it by itself: linear.py, _frozen_key).
    decode_bf16: bool = False

    def __post_init__(self):
        if self.act_dtype not in (torch.float16, torch.bfloat16):
            raise ValueError(f"MixqConfig: act_dtype must be torch.float16 or torch.bfloat16, got {self.act_dtype}")

    def copy(self, **changes) -> "MixqConfig":
        return replace(self, **changes)

    def key(self):
        """What of the configuration is part of a kept plan's / joint image's identity."""
        return (self.pack_fmt, self.pack_fmt4, self.small_batch_m4, self.act_dtype)
