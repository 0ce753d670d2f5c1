// Internal interface between gemm.hip (dispatch) and gemm_skinny.hip (small-batch kernel).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "common.h"

bool mixq_skinny_applies(int bit, int M, int N, int KB, bool x_packed, bool w_packed);
int mixq_skinny_launch(const MixqFusedProblem& p, int bit, int wf16, hipStream_t st);
// the bfloat16 forms (gemm_skinny_bf16.hip): x_out / w_out, addend and y are bfloat16; the same problems as mixq_skinny_applies names
int mixq_skinny_launch_bf16(const MixqFusedProblem& p, int bit, int wf16, hipStream_t st);
