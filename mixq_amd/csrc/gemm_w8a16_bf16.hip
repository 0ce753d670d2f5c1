// The bf16 forms of the weight-only W8A16 kernels (x / addend / y in bfloat16: include/mixq_hip.h, "bf16 weight-only layers") are
// gemm_w8a16.hip compiled a SECOND time with the container as a trailing template parameter: one source for both forms, two translation
// units, two GPU code objects.  The fp16 object then holds exactly the kernels, names and instructions it held before (its k loop sits at the
// edge of its register budget), and the two halves compile in parallel.
// Exports mixq_wo_bf16_kernel and mixq_wo_pack_s8; everything else of gemm_w8a16.hip - table, choice, launch, entry points - lives in its own object.
#define MIXQ_WO_BF16_TU 1
#include "gemm_w8a16.hip"
