// The bf16 forms of the joint gate / up launch (mixq_gemm_i8_pair_bf16 / mixq_gemm_i4_pair_bf16: include/mixq_hip.h, "ABI 1.5") are
// gemm_wreg.hip compiled a THIRD time: container bfloat16 (BF = true) and the paired epilogue (ABL = 90) together, nine kernels in a GPU
// code object of their own.  The fp16 object and gemm_wreg_bf16.hip's keep exactly the kernels, names and bytes they held (moving the fp16
// object's .text once cost the metric shape 2 %), and tools/check_wreg_asm.py lists these nine under this file's name only.
// Exports mixq_wr_bf16_pair_kernel (gemm_wreg.h); table, choice and launch live in gemm_wreg.hip's own object.
#define MIXQ_WR_BF16_TU 2
#include "gemm_wreg.hip"
