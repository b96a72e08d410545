// Tuning knobs.  The product library (disn_amd/csrc/build.py, default) has NONE and reads no environment variable.
// `build.py --tuning` compiles the same sources with -DDISN_TUNING into libdisn_amd_tuning.so, where the three knobs
// below exist as run-time values behind the extra exports disn_tuning_set() / disn_tuning_set_ptr() (api.hip); only
// tools/ and the counted-waits test load that library.  Every read of a knob sits inside #ifdef DISN_TUNING.
#pragma once

#ifdef DISN_TUNING
namespace disn {
namespace tune {
extern int fused_safe;         // key 0 -- 1: the fused point MLP waits for ALL LDS-DMA at every sync (tools/fused_check.py)
extern int aux_cu_mode;        // key 1 -- > 0: disn_ctx_create puts the auxiliary stream on a CU subset (hipExtStreamCreateWithCUMask)
extern long long* ch2_stamps;  // disn_tuning_set_ptr key 0 -- conv_h2 / conv_h2w kernels write 16 clock stamps per workgroup
                               // here (tools/conv_h2_stamps.py)
}  // namespace tune
}  // namespace disn
#endif
