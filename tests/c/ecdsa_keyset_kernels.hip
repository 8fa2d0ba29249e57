/* The two key-set kernels of bftkv_amd/csrc/ec_kernels.hip instantiated on all four curves and nothing else, so that
 * tests/test_ecdsa_keyset_reference.py can read their register and scratch figures from the compiler's remarks
 * (-Rpass-analysis=kernel-resource-usage, device code only) without compiling the whole library.  Test infrastructure only. */
#include <hip/hip_runtime.h>
#include "../../include/bftkv_gpu.h"
#include "../../bftkv_amd/csrc/mont28.h"        // MONT_N: the limb rows k_modinv exchanges with the k_ecv_* kernels
#include "../../bftkv_amd/csrc/ec_kernels.hip"

const void* const eks_kernels[8] = {
    (const void*)bftkv::k_ec_keytab_build<7>, (const void*)bftkv::k_ec_keytab_build<8>, (const void*)bftkv::k_ec_keytab_build<12>,
    (const void*)bftkv::k_ec_keytab_build<17>, (const void*)bftkv::k_ecv_key_tab<7>,     (const void*)bftkv::k_ecv_key_tab<8>,
    (const void*)bftkv::k_ecv_key_tab<12>,     (const void*)bftkv::k_ecv_key_tab<17>,
};
