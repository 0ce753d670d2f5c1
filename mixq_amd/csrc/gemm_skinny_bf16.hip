// The bf16 forms of the small-batch kernel (mixq_gemm_i8_decode_bf16 / mixq_gemm_i4_decode_bf16: include/mixq_hip.h, "bf16 small-batch form
// (ABI 1.7)") are gemm_skinny.hip compiled a SECOND time with the container as a trailing template parameter: one source for both forms, two
// translation units, two GPU code objects.  The fp16 object then holds exactly the kernels, names and bytes it held before.
// Exports mixq_skinny_launch_bf16 (gemm_skinny.h); mixq_skinny_applies and the fp16 launch live in gemm_skinny.hip's own object.
#define MIXQ_SKINNY_BF16_TU 1
#include "gemm_skinny.hip"
