// The bf16 forms of the weights-in-registers kernels (x_out / w_out / addend / y in bfloat16: include/mixq_hip.h, "bf16 layers") are
// gemm_wreg.hip compiled a SECOND time with the container as a trailing template parameter: one source for both forms, two translation
// units, two GPU code objects.  The fp16 object then holds exactly the kernels, names and bytes it held before (see the note at the
// kernel's template head: moving its .text costs the metric shape 2 %), and the two halves compile in parallel.
// Exports mixq_wr_bf16_kernel (gemm_wreg.h); everything else of gemm_wreg.hip - table, choice, launch - lives in its own object.
#define MIXQ_WR_BF16_TU 1
#include "gemm_wreg.hip"
