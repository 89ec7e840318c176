#pragma clang fp contract(off)
// ^ first, and at file scope, so it holds for everything after it in the including translation unit: the fp32 step arithmetic of
// sampler.hip and fifo.hip.  The reference evaluates these expressions as separate fp32 torch ops (mul, sub, div ...), and the tests
// compare with torch.equal; one fused multiply-add changes the last bit.  The Makefile passes -ffp-contract=off for both files too,
// but a helper moved to another file or a build that bypasses the Makefile must not contract silently.
// Device-inline only: formulas that sampler.hip and fifo.hip both evaluate.
#pragma once

// classifier-free guidance, ddim.py:304 / :372: e_t = e_u + s (e_c - e_u)
__device__ __forceinline__ float cfg_guidance(float e_c, float e_u, float scale) { return e_u + scale * (e_c - e_u); }
