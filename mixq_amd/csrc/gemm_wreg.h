// Internal interface between gemm.hip (dispatch) and gemm_wreg.hip (weights-in-registers kernels, MIXQ_FMT_F16X64 operands).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "common.h"

int mixq_wr_num_configs();
int mixq_wr_set_krot(int v);                 // k-step rotation between neighbouring N tiles (tuning; results do not depend on it)
const char* mixq_wr_config_name(int c);
// config for (M, N, KB) or -1 when the data-parallel kernels of gemm.hip should run instead
int mixq_wr_pick(int bit, int M, int N, int KB);
// one launch of tiling c over the weight rows [n_begin, n_begin + n_cols) of problem p (only the launch that ends at p.N may hold a partial
// tile); bit: 8, 4, or 6 (int4 as FP6 codes).  p.bf16 with a tiling without a bf16 form (of the paired epilogue, when p.act asks for it): MIXQ_EINVAL
int mixq_wr_launch(const MixqFusedProblem& p, int c, int bit, unsigned long long* trace, hipStream_t st, int n_begin, int n_cols);
// the bf16 forms: the tiling for a problem (-1: none), and whether a (forced) configuration has one
int mixq_wr_pick_bf16(int bit, int M, int N, int KB);   // bit: 8, or 6 (int4 as FP6 codes)
bool mixq_wr_has_bf16(int bit, int c);
const void* mixq_wr_bf16_kernel(int bit, int c);        // gemm_wreg_bf16.hip: the launch handle of tiling c's bf16 form, or nullptr
// N split for a partial last round of tiles: true when running tiling c over the first *n1 weight rows and tiling *c2 over the rest is priced
// cheaper than one launch of c (gemm_wreg.hip)
bool mixq_wr_split(int bit, int M, int N, int KB, int c, int* n1, int* c2);
// pairwise split-K form (two workgroups per 128 x 128 tile, half of K each, int32 hand-off through the registered workspace)
int mixq_wr_ksplit_config();                 // its configuration index
int mixq_wr_ksplit_ok(int M, int N, int KB); // MIXQ_OK when it can run this problem on the current device (workspace, residency), else the reason
bool mixq_wr_ksplit_pays(int M, int N, int KB);   // ... and the tile model says it is the faster choice
// the joint gate_proj / up_proj form (MIXQ_ACT_SILU_PAIR: interleaved weight rows, N / 2 output columns): the tiling for a problem, and
// whether a (forced) configuration has the paired epilogue
int mixq_wr_pick_pair(int bit, int M, int N, int KB);   // bit: 8, or 6 (int4 as FP6 codes)
bool mixq_wr_has_pair(int bit, int c);
// ... in bfloat16 (the `_pair_bf16` entry points): the pick (-1: none), whether a (forced) configuration has the form, and its launch handle
int mixq_wr_pick_pair_bf16(int bit, int M, int N, int KB);
bool mixq_wr_has_pair_bf16(int bit, int c);
const void* mixq_wr_bf16_pair_kernel(int bit, int c);   // gemm_wreg_bf16_pair.hip
