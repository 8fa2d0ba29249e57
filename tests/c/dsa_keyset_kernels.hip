/* The two key-set kernels of bftkv_amd/csrc/dsa_verify_kernels.hip instantiated in their one lane form, <19, 4>, and no other
 * template of that file (the non-template kernels of the two files included before it are compiled along), so that
 * tests/test_dsa_keyset_reference.py can read their register and scratch figures from the compiler's remarks
 * (-Rpass-analysis=kernel-resource-usage, device code only) without compiling the whole library.  The two files included first
 * are the ones capi.hip includes before it (the block size, ModTab and the multiplier).  Test infrastructure only. */
#include <hip/hip_runtime.h>
#include "../../include/bftkv_gpu.h"
#include "../../bftkv_amd/csrc/kernels.hip"
#include "../../bftkv_amd/csrc/threshold_kernels.hip"
#include "../../bftkv_amd/csrc/dsa_verify_kernels.hip"

const void* const dks_kernels[2] = {
    (const void*)bftkv::k_dsav_comb_build<bftkv::MONT_L, bftkv::MONT_TPI>,
    (const void*)bftkv::k_dsav_comb_exp<bftkv::MONT_L, bftkv::MONT_TPI>,
};
