// Diagnostic builds only (`make stamps` / `gndiag` / `diagx`): the GEMM translation units as ONE unit, so that their -D flags reach
// every kernel family and moca_debug_stamps (gemm.hip) reads the one g_stamps buffer that every stamped kernel writes -- without
// relocatable device code a __device__ array is per translation unit.  The product library never compiles this file.
#ifndef MOCA_DIAG_NAME
#error "gemm_diag.hip is the unit of the diagnostic builds: compile it with -DMOCA_DIAG_NAME"
#endif
#include "gemm.hip"
#include "gemm_tiled.hip"
#include "gemm_persistent.hip"
#include "gemm_halo.hip"
