"""ctypes binding of libbftkv_gpu.so (include/bftkv_gpu.h).

The product path has NO CPU fallback: if the HIP library is missing or no GPU is present, loading /
``Context()`` raises.  Nothing here imports ``oracle/``.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libbftkv_gpu.so")


class NativeError(RuntimeError):
    pass


class PubKey(C.Structure):
    _fields_ = [("key_id", C.c_uint64), ("entity_id", C.c_uint64), ("pk_algo", C.c_uint8),
                ("usable_sign", C.c_uint8), ("reserved", C.c_uint8 * 6),
                ("n", C.c_void_p), ("n_len", C.c_uint32), ("e", C.c_void_p), ("e_len", C.c_uint32),
                ("g", C.c_void_p), ("g_len", C.c_uint32), ("y", C.c_void_p), ("y_len", C.c_uint32)]


class QC(C.Structure):
    _fields_ = [("f", C.c_int32), ("min", C.c_int32), ("threshold", C.c_int32), ("suff", C.c_int32),
                ("node_ids", C.c_void_p), ("n_nodes", C.c_uint32)]


EXPORTS = [
    "bftkv_gpu_init", "bftkv_gpu_destroy", "bftkv_gpu_last_error", "bftkv_gpu_error_string",
    "bftkv_gpu_keyring_set", "bftkv_gpu_quorum_create", "bftkv_gpu_quorum_destroy",
    "bftkv_gpu_collective_verify", "bftkv_gpu_collective_verify_dev", "bftkv_gpu_sync",
    "bftkv_gpu_signature_verify", "bftkv_gpu_last_statuses", "bftkv_gpu_last_counters",
    "bftkv_gpu_signers", "bftkv_gpu_quorum_tally", "bftkv_gpu_modexp", "bftkv_gpu_last_timing",
    "bftkv_gpu_stream", "bftkv_gpu_modmul_product", "bftkv_gpu_lagrange_combine", "bftkv_gpu_dsa_calculate_r", "bftkv_gpu_selftest_reduce",
    "bftkv_gpu_comm_unique_id", "bftkv_gpu_comm_init", "bftkv_gpu_allgather_verdicts", "bftkv_gpu_sss_distribute", "bftkv_gpu_modinv",
    "bftkv_gpu_batcher_create", "bftkv_gpu_batcher_destroy", "bftkv_gpu_batcher_collective_verify",
    "bftkv_gpu_batcher_signature_verify", "bftkv_gpu_batcher_stats", "bftkv_gpu_set_dsa_window_bits", "bftkv_gpu_dsa_window_bits", "bftkv_gpu_set_dsa_table_budget", "bftkv_gpu_dsa_table_bytes", "bftkv_gpu_collective_verify_segments", "bftkv_gpu_message_verify", "bftkv_gpu_batcher_message_verify",
    "bftkv_gpu_modexp_ops", "bftkv_gpu_allgather_errs_dev", "bftkv_gpu_set_early_exit", "bftkv_gpu_last_sclk_mhz", "bftkv_gpu_last_plan_report", "bftkv_gpu_modmul_product_dev", "bftkv_gpu_lagrange_combine_dev",
    "bftkv_gpu_dsa_calculate_r_dev", "bftkv_gpu_sss_distribute_dev", "bftkv_gpu_modinv_dev",
    "bftkv_gpu_ctx_fork", "bftkv_gpu_batcher_create_lanes", "bftkv_gpu_batcher_times", "bftkv_gpu_comm_library", "bftkv_gpu_comm_selftest",
    "bftkv_gpu_collective_verify_small", "bftkv_gpu_signature_verify_small", "bftkv_gpu_set_hash_policy", "bftkv_gpu_signers_fenced",
    "bftkv_gpu_set_host_pipeline", "bftkv_gpu_batcher_cert_verify", "bftkv_gpu_host_pipeline_trace",
    "bftkv_gpu_batcher_cert_entity", "bftkv_gpu_set_lagrange_x_bound", "bftkv_gpu_batcher_modmul_product", "bftkv_gpu_batcher_lagrange_combine", "bftkv_gpu_batcher_dsa_calculate_r", "bftkv_gpu_batcher_modexp",
    "bftkv_gpu_ecdsa_calculate_r", "bftkv_gpu_ecdsa_calculate_r_dev", "bftkv_gpu_batcher_ecdsa_calculate_r", "bftkv_gpu_ec_scalar_base_mult",
    "bftkv_gpu_ecdsa_verify", "bftkv_gpu_ecdsa_verify_dev", "bftkv_gpu_batcher_ecdsa_verify",
    "bftkv_gpu_dsa_verify", "bftkv_gpu_dsa_verify_dev", "bftkv_gpu_batcher_dsa_verify",
    "bftkv_gpu_ecdsa_keyset_create", "bftkv_gpu_ecdsa_keyset_destroy", "bftkv_gpu_ecdsa_keyset_info", "bftkv_gpu_ecdsa_verify_keyset",
    "bftkv_gpu_ecdsa_verify_keyset_dev", "bftkv_gpu_batcher_ecdsa_verify_keyset", "bftkv_gpu_selftest_ecdsa_keyset_table",
    "bftkv_gpu_dsa_keyset_create", "bftkv_gpu_dsa_keyset_destroy", "bftkv_gpu_dsa_keyset_info", "bftkv_gpu_dsa_verify_keyset",
    "bftkv_gpu_dsa_verify_keyset_dev", "bftkv_gpu_batcher_dsa_verify_keyset", "bftkv_gpu_selftest_dsa_keyset_table",
    "bftkv_gpu_rsa_verify", "bftkv_gpu_rsa_verify_dev", "bftkv_gpu_rsa_keyset_create", "bftkv_gpu_rsa_keyset_destroy", "bftkv_gpu_rsa_keyset_info",
    "bftkv_gpu_rsa_verify_keyset", "bftkv_gpu_rsa_verify_keyset_dev", "bftkv_gpu_batcher_rsa_verify", "bftkv_gpu_batcher_rsa_verify_keyset",
    "bftkv_gpu_tpa_yi", "bftkv_gpu_tpa_bi", "bftkv_gpu_tpa_ni", "bftkv_gpu_batcher_tpa_yi", "bftkv_gpu_batcher_tpa_bi",
    "bftkv_gpu_rsa_partial_sign", "bftkv_gpu_batcher_rsa_partial_sign",
    "bftkv_gpu_tdsa_share", "bftkv_gpu_tdsa_share_dev", "bftkv_gpu_tecdsa_share", "bftkv_gpu_tecdsa_share_dev", "bftkv_gpu_tsig_partial_s",
    "bftkv_gpu_batcher_tdsa_share", "bftkv_gpu_batcher_tecdsa_share",
    "bftkv_gpu_rsa_signer_create", "bftkv_gpu_rsa_signer_destroy", "bftkv_gpu_rsa_signer_info", "bftkv_gpu_rsa_sign_keyset",
    "bftkv_gpu_rsa_sign_keyset_dev", "bftkv_gpu_selftest_rsa_crt", "bftkv_gpu_batcher_rsa_sign_keyset",
]

_lib = None


def load_library() -> C.CDLL:
    """dlopen the in-tree HIP library; raises NativeError when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise NativeError("%s not built -- run `python -c 'import __graft_entry__ as g; g.build()'`" % LIB_PATH)
    lib = C.CDLL(LIB_PATH)
    vp, u32, u64p, u8p = C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p
    lib.bftkv_gpu_init.argtypes = [C.c_int, C.POINTER(vp)]
    lib.bftkv_gpu_destroy.argtypes = [vp]
    lib.bftkv_gpu_destroy.restype = None
    lib.bftkv_gpu_last_error.argtypes = [vp]
    lib.bftkv_gpu_last_error.restype = C.c_char_p
    lib.bftkv_gpu_error_string.argtypes = [C.c_int]
    lib.bftkv_gpu_error_string.restype = C.c_char_p
    lib.bftkv_gpu_keyring_set.argtypes = [vp, C.POINTER(PubKey), u32]
    lib.bftkv_gpu_set_dsa_window_bits.argtypes = [vp, u32]
    lib.bftkv_gpu_dsa_window_bits.argtypes = [vp, C.POINTER(u32)]
    lib.bftkv_gpu_set_dsa_table_budget.argtypes = [vp, C.c_uint64]
    lib.bftkv_gpu_dsa_table_bytes.argtypes = [vp, C.POINTER(C.c_uint64), C.POINTER(u32)]
    lib.bftkv_gpu_set_hash_policy.argtypes = [vp, C.c_int, C.c_int]
    lib.bftkv_gpu_message_verify.argtypes = [vp, u32, vp, vp, vp, vp, vp, vp, C.c_uint64, vp, vp, vp]
    lib.bftkv_gpu_quorum_create.argtypes = [vp, C.POINTER(QC), u32, C.POINTER(C.c_int)]
    lib.bftkv_gpu_quorum_destroy.argtypes = [vp, C.c_int]
    lib.bftkv_gpu_collective_verify.argtypes = [vp, C.c_int, u32, u8p, u64p, u8p, u64p, u8p, vp, u8p, u8p]
    lib.bftkv_gpu_collective_verify_segments.argtypes = [vp, C.c_int, u32, u8p, u64p, u8p, u64p, u32, vp, u8p, u64p, u8p, vp, u8p, u8p]
    lib.bftkv_gpu_collective_verify_dev.argtypes = [vp, C.c_int, u32, u8p, u64p, u8p, u64p, C.c_uint64, u8p, vp, u8p, u8p]
    lib.bftkv_gpu_collective_verify_small.argtypes = [vp, C.c_int, u32, u8p, u64p, u8p, u64p, u8p, u8p]
    lib.bftkv_gpu_signature_verify_small.argtypes = [vp, u32, u8p, u64p, u8p, u64p, u64p, u8p, u8p]
    lib.bftkv_gpu_sync.argtypes = [vp]
    lib.bftkv_gpu_signature_verify.argtypes = [vp, u32, u8p, u64p, u8p, u64p, u64p, u8p, u8p]
    lib.bftkv_gpu_last_statuses.argtypes = [vp, u8p, vp, u32, C.POINTER(u32)]
    lib.bftkv_gpu_last_counters.argtypes = [vp, C.POINTER(C.c_uint64)]
    lib.bftkv_gpu_signers.argtypes = [vp, u32, u8p, u64p, u64p, u64p, C.c_uint64]
    lib.bftkv_gpu_signers_fenced.argtypes = [vp, u32, u8p, u64p, u64p, u64p, C.c_uint64, u8p]
    lib.bftkv_gpu_quorum_tally.argtypes = [vp, C.c_int, u32, u64p, u64p, u8p]
    lib.bftkv_gpu_modexp.argtypes = [vp, u32, u8p, u32, vp, u32, u8p, u8p, u32, u8p]
    lib.bftkv_gpu_last_timing.argtypes = [vp, C.POINTER(C.c_float)]
    lib.bftkv_gpu_modmul_product.argtypes = [vp, u32, u32, u8p, u32, vp, u32, u8p, u8p]
    lib.bftkv_gpu_lagrange_combine.argtypes = [vp, u32, u32, vp, u8p, u32, vp, u32, u8p, u8p, u8p]
    lib.bftkv_gpu_dsa_calculate_r.argtypes = [vp, u32, u32, vp, u8p, u32, u8p, u32, vp, u32, u8p, u8p, u8p, u8p]
    lib.bftkv_gpu_stream.argtypes = [vp]
    lib.bftkv_gpu_batcher_create.argtypes = [vp, u32, u32]
    lib.bftkv_gpu_batcher_create.restype = vp
    lib.bftkv_gpu_batcher_create_lanes.argtypes = [vp, u32, u32, u32]
    lib.bftkv_gpu_batcher_create_lanes.restype = vp
    lib.bftkv_gpu_ctx_fork.argtypes = [vp, C.POINTER(vp)]
    lib.bftkv_gpu_batcher_destroy.argtypes = [vp]
    lib.bftkv_gpu_batcher_destroy.restype = None
    lib.bftkv_gpu_batcher_collective_verify.argtypes = [vp, C.c_int, C.c_char_p, C.c_uint64, C.c_char_p, C.c_uint64, u8p, u8p]
    lib.bftkv_gpu_batcher_signature_verify.argtypes = [vp, C.c_char_p, C.c_uint64, C.c_char_p, C.c_uint64, vp, u8p, u8p]
    lib.bftkv_gpu_batcher_cert_verify.argtypes = [vp, C.c_char_p, C.c_uint64, C.c_char_p, C.c_uint64, C.c_char_p, C.c_uint64, u8p, u8p, vp, u8p]
    lib.bftkv_gpu_set_lagrange_x_bound.argtypes = [vp, u32]
    lib.bftkv_gpu_batcher_cert_entity.argtypes = [vp, C.c_char_p, C.c_uint64, u8p, u8p, vp, u8p, vp, vp, vp, u32, vp]
    lib.bftkv_gpu_batcher_message_verify.argtypes = [vp, C.c_char_p, C.c_uint64, vp, vp, vp, vp, C.c_uint64, vp, vp, vp]
    lib.bftkv_gpu_batcher_stats.argtypes = [vp, C.POINTER(C.c_uint64)]
    lib.bftkv_gpu_batcher_modmul_product.argtypes = [vp, u32, u8p, u32, u8p, u8p, u8p]
    lib.bftkv_gpu_batcher_lagrange_combine.argtypes = [vp, u32, vp, u8p, u32, u8p, u8p, u8p]
    lib.bftkv_gpu_batcher_dsa_calculate_r.argtypes = [vp, u32, vp, u8p, u32, u8p, u32, u8p, u8p, u8p, u8p]
    lib.bftkv_gpu_batcher_modexp.argtypes = [vp, u8p, u32, u8p, u32, u8p, u8p, u8p]
    lib.bftkv_gpu_batcher_times.argtypes = [vp, C.POINTER(C.c_uint64)]
    lib.bftkv_gpu_sss_distribute.argtypes = [vp, u32, u32, u32, u8p, u32, vp, u32, u8p, u8p]
    lib.bftkv_gpu_modinv.argtypes = [vp, u32, u8p, u32, vp, u32, u8p, u8p, u8p]
    lib.bftkv_gpu_comm_unique_id.argtypes = [u8p]
    lib.bftkv_gpu_comm_init.argtypes = [vp, C.c_int, C.c_int, u8p]
    lib.bftkv_gpu_comm_library.argtypes = [C.c_char_p, u32, C.POINTER(C.c_int)]
    lib.bftkv_gpu_comm_selftest.argtypes = [vp, u32, C.POINTER(u32)]
    lib.bftkv_gpu_allgather_verdicts.argtypes = [vp, u8p, C.c_uint64, u8p]
    lib.bftkv_gpu_stream.restype = vp
    lib.bftkv_gpu_set_early_exit.argtypes = [vp, C.c_int]
    lib.bftkv_gpu_set_host_pipeline.argtypes = [vp, u32]
    lib.bftkv_gpu_host_pipeline_trace.argtypes = [vp, C.POINTER(C.c_float), u32, C.POINTER(u32)]
    lib.bftkv_gpu_last_sclk_mhz.argtypes = [vp, C.POINTER(C.c_float)]
    lib.bftkv_gpu_last_plan_report.argtypes = [vp, C.POINTER(u32), u32, C.POINTER(u32)]
    lib.bftkv_gpu_modexp_ops.argtypes = lib.bftkv_gpu_modexp.argtypes
    lib.bftkv_gpu_allgather_errs_dev.argtypes = [vp, u8p, u32, u32, u8p]
    lib.bftkv_gpu_modmul_product_dev.argtypes = lib.bftkv_gpu_modmul_product.argtypes
    lib.bftkv_gpu_lagrange_combine_dev.argtypes = lib.bftkv_gpu_lagrange_combine.argtypes
    lib.bftkv_gpu_dsa_calculate_r_dev.argtypes = lib.bftkv_gpu_dsa_calculate_r.argtypes
    lib.bftkv_gpu_sss_distribute_dev.argtypes = lib.bftkv_gpu_sss_distribute.argtypes
    lib.bftkv_gpu_modinv_dev.argtypes = lib.bftkv_gpu_modinv.argtypes
    lib.bftkv_gpu_ecdsa_calculate_r.argtypes = [vp, u32, u32, vp, u8p, u8p, u8p, u32, u8p, u8p]
    lib.bftkv_gpu_ecdsa_calculate_r_dev.argtypes = lib.bftkv_gpu_ecdsa_calculate_r.argtypes
    lib.bftkv_gpu_batcher_ecdsa_calculate_r.argtypes = [vp, u32, vp, u8p, u8p, u8p, u32, u8p, u8p]
    lib.bftkv_gpu_ec_scalar_base_mult.argtypes = [vp, u32, u8p, u32, u8p, u32, u8p, u8p]
    lib.bftkv_gpu_ecdsa_verify.argtypes = [vp, u32, u8p, u32, u8p, vp, u32, u8p, u8p, u32, u8p, u8p]
    lib.bftkv_gpu_ecdsa_verify_dev.argtypes = lib.bftkv_gpu_ecdsa_verify.argtypes
    lib.bftkv_gpu_batcher_ecdsa_verify.argtypes = [vp, u8p, u32, u8p, u8p, u8p, u32, u8p, u8p]
    lib.bftkv_gpu_dsa_verify.argtypes = [vp, u32, u8p, u32, u8p, u32, vp, u32, u8p, vp, u32, u32, u8p, u8p, u8p, u8p, u8p]
    lib.bftkv_gpu_dsa_verify_dev.argtypes = lib.bftkv_gpu_dsa_verify.argtypes
    lib.bftkv_gpu_batcher_dsa_verify.argtypes = [vp, u8p, u32, u8p, u32, u8p, u32, u8p, u8p, u8p, u8p, u8p]
    lib.bftkv_gpu_ecdsa_keyset_create.argtypes = [vp, u32, u8p, u8p, u32, C.POINTER(C.c_int)]
    lib.bftkv_gpu_ecdsa_keyset_destroy.argtypes = [vp, C.c_int]
    lib.bftkv_gpu_ecdsa_keyset_info.argtypes = [vp, C.c_int, C.POINTER(u32), C.POINTER(u32), C.POINTER(u32), C.POINTER(C.c_uint64)]
    lib.bftkv_gpu_ecdsa_verify_keyset.argtypes = [vp, C.c_int, u32, u8p, u32, u8p, vp, u8p, u8p]
    lib.bftkv_gpu_ecdsa_verify_keyset_dev.argtypes = lib.bftkv_gpu_ecdsa_verify_keyset.argtypes
    lib.bftkv_gpu_batcher_ecdsa_verify_keyset.argtypes = [vp, C.c_int, u32, u8p, u32, u8p, u8p, u8p]
    lib.bftkv_gpu_selftest_ecdsa_keyset_table.argtypes = [vp, C.c_int, u32, vp, C.c_uint64]
    lib.bftkv_gpu_dsa_keyset_create.argtypes = [vp, u32, u8p, vp, u32, u32, u8p, u8p, u8p, u32, u32, C.POINTER(C.c_int)]
    lib.bftkv_gpu_dsa_keyset_destroy.argtypes = [vp, C.c_int]
    lib.bftkv_gpu_dsa_keyset_info.argtypes = [vp, C.c_int] + [C.POINTER(u32)] * 6 + [C.POINTER(C.c_uint64)]
    lib.bftkv_gpu_dsa_verify_keyset.argtypes = [vp, C.c_int, u32, u8p, u32, u8p, vp, u8p, u8p]
    lib.bftkv_gpu_dsa_verify_keyset_dev.argtypes = lib.bftkv_gpu_dsa_verify_keyset.argtypes
    lib.bftkv_gpu_batcher_dsa_verify_keyset.argtypes = [vp, C.c_int, u32, u8p, u32, u8p, u8p, u8p]
    lib.bftkv_gpu_selftest_dsa_keyset_table.argtypes = [vp, C.c_int, u32, vp, C.c_uint64]
    lib.bftkv_gpu_rsa_verify.argtypes = [vp, u32, u8p, u32, u32, u8p, u32, vp, u32, u8p, vp, u8p, u8p]
    lib.bftkv_gpu_rsa_verify_dev.argtypes = lib.bftkv_gpu_rsa_verify.argtypes
    lib.bftkv_gpu_rsa_keyset_create.argtypes = [vp, u32, u8p, vp, u32, C.POINTER(C.c_int)]
    lib.bftkv_gpu_rsa_keyset_destroy.argtypes = [vp, C.c_int]
    lib.bftkv_gpu_rsa_keyset_info.argtypes = [vp, C.c_int] + [C.POINTER(u32)] * 3
    lib.bftkv_gpu_rsa_verify_keyset.argtypes = [vp, C.c_int, u32, u8p, u32, u32, u8p, vp, u8p, u8p]
    lib.bftkv_gpu_rsa_verify_keyset_dev.argtypes = lib.bftkv_gpu_rsa_verify_keyset.argtypes
    lib.bftkv_gpu_batcher_rsa_verify.argtypes = [vp, u8p, u32, u32, u8p, u32, u8p, u32, u8p, u8p]
    lib.bftkv_gpu_batcher_rsa_verify_keyset.argtypes = [vp, C.c_int, u32, u8p, u32, u32, u8p, u8p, u8p]
    lib.bftkv_gpu_tpa_yi.argtypes = [vp, u32, u8p, u32, u8p, u32, vp, u32, u8p, u8p, u8p]
    lib.bftkv_gpu_tpa_bi.argtypes = [vp, u32, u8p, u8p, vp, u32, u8p, u32, u8p, u32, vp, u32, u8p, u8p, u8p, u8p, u8p]
    lib.bftkv_gpu_tpa_ni.argtypes = [vp, u32, u8p, u8p, vp, u32, u8p, u32, u8p, u32, vp, u32, u8p, u8p, u8p, u8p]
    lib.bftkv_gpu_batcher_tpa_yi.argtypes = [vp, u8p, u32, u8p, u32, u8p, u8p, u8p]
    lib.bftkv_gpu_batcher_tpa_bi.argtypes = [vp, u8p, u8p, u32, u32, u8p, u32, u8p, u32, u8p, u8p, u8p, u8p, u8p]
    lib.bftkv_gpu_rsa_partial_sign.argtypes = [vp, u32, u8p, u32, vp, vp, u32, u8p, u32, u32, vp, u8p, u32, vp, u8p, u8p, u8p]
    lib.bftkv_gpu_batcher_rsa_partial_sign.argtypes = [vp, u8p, u32, u8p, u32, u32, u8p, u32, vp, u8p, u8p, u8p]
    lib.bftkv_gpu_tdsa_share.argtypes = [vp, C.c_int, u32, vp, u32, u8p, u8p, u8p, u8p, u8p, u8p]
    lib.bftkv_gpu_tdsa_share_dev.argtypes = lib.bftkv_gpu_tdsa_share.argtypes
    lib.bftkv_gpu_tecdsa_share.argtypes = [vp, u32, u32, u8p, u8p, u32, u8p, u8p, u8p, u8p, u8p]
    lib.bftkv_gpu_tecdsa_share_dev.argtypes = lib.bftkv_gpu_tecdsa_share.argtypes
    lib.bftkv_gpu_tsig_partial_s.argtypes = [vp, u32, u8p, u8p, u8p, u8p, u8p, u32, vp, u32, u8p, u8p, u8p]
    lib.bftkv_gpu_batcher_tdsa_share.argtypes = [vp, C.c_int, u32, u32, u8p, u32, u32, u8p, u8p, u8p, u8p, u8p]
    lib.bftkv_gpu_batcher_tecdsa_share.argtypes = [vp, u32, u8p, u8p, u32, u8p, u8p, u8p, u8p, u8p]
    lib.bftkv_gpu_rsa_signer_create.argtypes = [vp, u32, u8p, vp, u32, u8p, u8p, u8p, u8p, u8p, u32, C.POINTER(C.c_int)]
    lib.bftkv_gpu_rsa_signer_destroy.argtypes = [vp, C.c_int]
    lib.bftkv_gpu_rsa_signer_info.argtypes = [vp, C.c_int] + [C.POINTER(u32)] * 4
    lib.bftkv_gpu_rsa_sign_keyset.argtypes = [vp, C.c_int, u32, u8p, u32, u32, vp, u8p, u8p]
    lib.bftkv_gpu_rsa_sign_keyset_dev.argtypes = [vp, C.c_int, u32, vp, u32, u32, vp, vp, vp]
    lib.bftkv_gpu_selftest_rsa_crt.argtypes = [vp, C.c_int, u32, u8p, vp, u8p, u8p]
    lib.bftkv_gpu_batcher_rsa_sign_keyset.argtypes = [vp, C.c_int, u32, u8p, u32, u32, u8p, u8p]
    for name in EXPORTS:
        if name not in ("bftkv_gpu_destroy", "bftkv_gpu_last_error", "bftkv_gpu_error_string", "bftkv_gpu_stream",
                        "bftkv_gpu_batcher_create", "bftkv_gpu_batcher_create_lanes", "bftkv_gpu_batcher_destroy"):
            getattr(lib, name).restype = C.c_int
    _lib = lib
    return lib


def _ptr(a: Optional[np.ndarray]):
    if a is None:
        return None
    assert a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(C.c_void_p)


class Context:
    """One verifier context = one GPU + one HIP stream (bftkv_gpu_init)."""

    def __init__(self, device: int = 0):
        self.lib = load_library()
        h = C.c_void_p()
        rc = self.lib.bftkv_gpu_init(device, C.byref(h))
        if rc != 0:
            raise NativeError("bftkv_gpu_init(device=%d) failed with %d: no usable MI355X / HIP runtime "
                              "(there is no CPU fallback)" % (device, rc))
        self.h = h
        self._keep = []

    def close(self):
        if self.h:
            self.lib.bftkv_gpu_destroy(self.h)
            self.h = None

    def set_hash_policy(self, hash_id: int, state: int):
        """bftkv_gpu_set_hash_policy: MD5 (1) / RIPEMD-160 (3): 0 unknown (fenced), 1 available, 2 not available."""
        self._check(self.lib.bftkv_gpu_set_hash_policy(self.h, hash_id, state), "set_hash_policy")

    def fork(self) -> "Context":
        """bftkv_gpu_ctx_fork: a context with its own streams and arena over this one's key table and quorums
        (verify calls only; close it before its root)."""
        h = C.c_void_p()
        self._check(self.lib.bftkv_gpu_ctx_fork(self.h, C.byref(h)), "ctx_fork")
        f = Context.__new__(Context)
        f.lib, f.h, f._keep, f.root = self.lib, h, [], self
        return f

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc: int, what: str):
        if rc != 0:
            raise NativeError("%s failed (%d): %s" % (what, rc, self.lib.bftkv_gpu_last_error(self.h).decode()))

    # ---- keyring
    def keyring_set(self, keys):
        """keys: iterable of dicts {key_id, entity_id, pk_algo, usable_sign, n, e[, g, y]} with
        big-endian ``bytes`` material, in keyring order."""
        keys = list(keys)
        arr = (PubKey * max(1, len(keys)))()
        bufs = []
        for i, k in enumerate(keys):
            arr[i].key_id = k["key_id"]
            arr[i].entity_id = k.get("entity_id", k["key_id"])
            arr[i].pk_algo = k["pk_algo"]
            arr[i].usable_sign = 1 if k.get("usable_sign", True) else 0
            for name in ("n", "e", "g", "y"):
                b = k.get(name) or b""
                cb = C.create_string_buffer(b, len(b)) if b else None
                bufs.append(cb)
                setattr(arr[i], name, C.cast(cb, C.c_void_p) if cb is not None else None)
                setattr(arr[i], name + "_len", len(b))
        self._check(self.lib.bftkv_gpu_keyring_set(self.h, arr, len(keys)), "keyring_set")

    def message_verify(self, messages):
        """Signature half of PGPMessage.Decrypt for a batch of already-decrypted packet sequences (bftkv_gpu_message_verify).
        Returns (status[n], signer_key_id[n], peer_id[n], [plain bytes], [file name bytes])."""
        n = len(messages)
        blob = np.frombuffer(b"".join(messages), dtype=np.uint8) if n and sum(map(len, messages)) else np.zeros(1, dtype=np.uint8)
        off = np.zeros(n + 1, dtype=np.uint64)
        off[1:] = np.cumsum([len(m) for m in messages], dtype=np.uint64)
        st = np.zeros(max(1, n), dtype=np.uint8)
        signer = np.zeros(max(1, n), dtype=np.uint64)
        peer = np.zeros(max(1, n), dtype=np.uint64)
        plain = np.zeros(max(1, int(off[n])), dtype=np.uint8)
        poff = np.zeros(n + 1, dtype=np.uint64)
        fn = np.zeros((max(1, n), 256), dtype=np.uint8)
        fl = np.zeros(max(1, n), dtype=np.uint8)
        self._check(self.lib.bftkv_gpu_message_verify(self.h, n, _ptr(np.ascontiguousarray(blob)), _ptr(off), _ptr(st), _ptr(signer), _ptr(peer),
                                                      _ptr(plain), len(plain), _ptr(poff), _ptr(fn), _ptr(fl)), "message_verify")
        plains = [plain[int(poff[i]):int(poff[i + 1])].tobytes() for i in range(n)]
        names = [fn[i, :int(fl[i])].tobytes() for i in range(n)]
        return st[:n], signer[:n], peer[:n], plains, names

    def set_early_exit(self, on: bool) -> None:
        """collective_verify: stop verifying where the reference stops reading (default) / verify every packet."""
        self._check(self.lib.bftkv_gpu_set_early_exit(self.h, 1 if on else 0), "set_early_exit")

    def set_host_pipeline(self, pieces: int, copy: str = "", tight: bool = False) -> None:
        """collective_verify over host buffers: 0 = split big batches by size (default), 1 = never, 2..8 = that many pieces;
        copy = "direct" (hipMemcpyAsync from the caller's memory, the default) or "ring" (the library's page-locked staging ring)."""
        mode = {"": 0, "ring": 0x100, "direct": 0x200}[copy]
        self._check(self.lib.bftkv_gpu_set_host_pipeline(self.h, pieces | mode | (0x400 if tight else 0)), "set_host_pipeline")

    def host_pipeline_trace(self):
        """Host-side timeline (microseconds) of the last pipelined host-buffer call: see bftkv_gpu_host_pipeline_trace."""
        buf = (C.c_float * 96)()
        n = C.c_uint32(0)
        self._check(self.lib.bftkv_gpu_host_pipeline_trace(self.h, buf, 96, C.byref(n)), "host_pipeline_trace")
        v = [float(buf[i]) for i in range(min(96, n.value))]
        if not v:
            return None
        P = int(v[0])
        names = ("ss_enqueued", "payload_enqueued", "picked_up", "payload_hook", "enqueued", "drained", "gpu_start", "gpu_modexp_start", "gpu_modexp_end", "gpu_end")
        return {"pieces": P, "ring": bool(v[1]), "copiers_joined_us": v[2], "copy_stream_drained_us": v[3], "done_us": v[4], "largest_piece_items": int(v[5]), "second_passes": int(v[6]),
                "per_piece_us": [{nm: round(v[8 + 10 * k + j], 1) for j, nm in enumerate(names)} for k in range(P)]}

    def set_dsa_window_bits(self, bits: int) -> None:
        """Pin the DSA fixed-base table width (4 or 8 .. 20 bits; 0 = default policy); applies at the next keyring_set."""
        self._check(self.lib.bftkv_gpu_set_dsa_window_bits(self.h, bits), "set_dsa_window_bits")

    def dsa_window_bits(self) -> int:
        """The width the current key table's DSA tables were built at (0: no DSA key)."""
        b = C.c_uint32(0)
        self._check(self.lib.bftkv_gpu_dsa_window_bits(self.h, C.byref(b)), "dsa_window_bits")
        return int(b.value)

    def set_dsa_table_budget(self, nbytes: int) -> None:
        """Bound on the HBM the DSA tables may hold (0 = the free-memory policy); applies at the next keyring_set."""
        self._check(self.lib.bftkv_gpu_set_dsa_table_budget(self.h, int(nbytes)), "set_dsa_table_budget")

    def dsa_table_bytes(self):
        """(bytes of HBM the DSA tables hold, limbs per table entry: 76, or 112 with a key whose p exceeds 2048 bits)"""
        b, e = C.c_uint64(0), C.c_uint32(0)
        self._check(self.lib.bftkv_gpu_dsa_table_bytes(self.h, C.byref(b), C.byref(e)), "dsa_table_bytes")
        return int(b.value), int(e.value)

    # ---- quorum
    def quorum_create(self, qcs) -> int:
        """qcs: iterable of (f, min, threshold, suff, [node ids])."""
        qcs = list(qcs)
        arr = (QC * max(1, len(qcs)))()
        keep = []
        for i, (f, mn, thr, suff, nodes) in enumerate(qcs):
            ids = np.ascontiguousarray(np.array(list(nodes), dtype=np.uint64))
            keep.append(ids)
            arr[i].f, arr[i].min, arr[i].threshold, arr[i].suff = f, mn, thr, suff
            arr[i].node_ids = ids.ctypes.data if len(ids) else None
            arr[i].n_nodes = len(ids)
        out = C.c_int(-1)
        self._check(self.lib.bftkv_gpu_quorum_create(self.h, arr, len(qcs), C.byref(out)), "quorum_create")
        return out.value

    def quorum_destroy(self, q: int):
        self._check(self.lib.bftkv_gpu_quorum_destroy(self.h, q), "quorum_destroy")

    # ---- verification
    def collective_verify(self, quorum: int, tbs_blob, tbs_off, ss_blob, ss_off):
        n = len(tbs_off) - 1
        tbs_blob, ss_blob = _u8(tbs_blob), _u8(ss_blob)
        tbs_off, ss_off = _u64(tbs_off), _u64(ss_off)
        err = np.zeros(n, dtype=np.uint8)
        nver = np.zeros(n, dtype=np.uint32)
        verdict = np.zeros(n, dtype=np.uint8)
        self.last_fenced = np.zeros(n, dtype=np.uint8)       # fenced_out of this call (see include/bftkv_gpu.h "fenced inputs")
        small = self.collective_verify_small(quorum, tbs_blob, tbs_off, ss_blob, ss_off) if self._cross_check(n) else None
        self._check(self.lib.bftkv_gpu_collective_verify(self.h, quorum, n, _ptr(tbs_blob), _ptr(tbs_off), _ptr(ss_blob),
                                                         _ptr(ss_off), _ptr(err), _ptr(nver), _ptr(verdict), _ptr(self.last_fenced)),
                    "collective_verify")
        self._compare_small("collective_verify", small, err, self.last_fenced)
        return err, nver, verdict

    # The parity tests set check_small: every batched verify call is then ALSO made through the staged small-call route
    # (bftkv_gpu_*_verify_small -- midstates from the host, one stream, 8-lane modexp, every packet verified) first, and the two
    # answers must be identical item by item.
    check_small = False

    def collective_verify_segments(self, quorum: int, prefix_blob, prefix_off, shared_blob, shared_off, seg_of_item, ss_blob, ss_off):
        """bftkv_gpu_collective_verify_segments: payload i = prefix i || shared segment seg_of_item[i] (0xFFFFFFFF: none)."""
        n = len(prefix_off) - 1
        prefix_blob, shared_blob, ss_blob = _u8(prefix_blob), _u8(shared_blob), _u8(ss_blob)
        prefix_off, shared_off, ss_off = _u64(prefix_off), _u64(shared_off), _u64(ss_off)
        seg = np.ascontiguousarray(seg_of_item, dtype=np.uint32)
        err = np.zeros(n, dtype=np.uint8)
        nver = np.zeros(n, dtype=np.uint32)
        verdict = np.zeros(n, dtype=np.uint8)
        self.last_fenced = np.zeros(n, dtype=np.uint8)
        self._check(self.lib.bftkv_gpu_collective_verify_segments(self.h, quorum, n, _ptr(prefix_blob), _ptr(prefix_off), _ptr(shared_blob),
                                                                  _ptr(shared_off), len(shared_off) - 1, _ptr(seg), _ptr(ss_blob), _ptr(ss_off),
                                                                  _ptr(err), _ptr(nver), _ptr(verdict), _ptr(self.last_fenced)),
                    "collective_verify_segments")
        return err, nver, verdict

    def _cross_check(self, n: int) -> bool:
        return bool(self.check_small) and 0 < n <= 4096

    @staticmethod
    def _compare_small(what, small, err, fenced):
        if small is None:
            return
        e2, f2 = small
        if not (np.array_equal(e2, err) and np.array_equal(f2, fenced)):
            bad = [int(i) for i in np.nonzero((e2 != err) | (f2 != fenced))[0][:8]]
            raise NativeError("%s: the small-call route disagrees with the batched one at items %s: err %s vs %s, fenced %s vs %s"
                              % (what, bad, e2[bad].tolist(), err[bad].tolist(), f2[bad].tolist(), fenced[bad].tolist()))

    def collective_verify_small(self, quorum: int, tbs_blob, tbs_off, ss_blob, ss_off):
        """bftkv_gpu_collective_verify_small: (err, fenced)."""
        n = len(tbs_off) - 1
        tbs_blob, ss_blob = _u8(tbs_blob), _u8(ss_blob)
        tbs_off, ss_off = _u64(tbs_off), _u64(ss_off)
        err = np.zeros(n, dtype=np.uint8)
        fenced = np.zeros(n, dtype=np.uint8)
        self._check(self.lib.bftkv_gpu_collective_verify_small(self.h, quorum, n, _ptr(tbs_blob), _ptr(tbs_off), _ptr(ss_blob), _ptr(ss_off),
                                                               _ptr(err), _ptr(fenced)), "collective_verify_small")
        return err, fenced

    def signature_verify_small(self, tbs_blob, tbs_off, sig_blob, sig_off, cert_key_id=None):
        """bftkv_gpu_signature_verify_small: (err, fenced)."""
        n = len(tbs_off) - 1
        tbs_blob, sig_blob = _u8(tbs_blob), _u8(sig_blob)
        tbs_off, sig_off = _u64(tbs_off), _u64(sig_off)
        ck = None if cert_key_id is None else _u64(cert_key_id)
        err = np.zeros(n, dtype=np.uint8)
        fenced = np.zeros(n, dtype=np.uint8)
        self._check(self.lib.bftkv_gpu_signature_verify_small(self.h, n, _ptr(tbs_blob), _ptr(tbs_off), _ptr(sig_blob), _ptr(sig_off), _ptr(ck),
                                                              _ptr(err), _ptr(fenced)), "signature_verify_small")
        return err, fenced

    def collective_verify_dev(self, quorum: int, n_items: int, tbs_ptr: int, tbs_off_ptr: int, ss_ptr: int, ss_off_ptr: int,
                              ss_len: int, err_ptr: int, nver_ptr: int, verdict_ptr: int, fenced_ptr: int = 0):
        self._check(self.lib.bftkv_gpu_collective_verify_dev(self.h, quorum, n_items, tbs_ptr, tbs_off_ptr, ss_ptr, ss_off_ptr,
                                                             ss_len, err_ptr, nver_ptr, verdict_ptr, fenced_ptr or None), "collective_verify_dev")

    def sync(self):
        self._check(self.lib.bftkv_gpu_sync(self.h), "sync")

    def signature_verify(self, tbs_blob, tbs_off, sig_blob, sig_off, cert_key_id=None):
        n = len(tbs_off) - 1
        tbs_blob, sig_blob = _u8(tbs_blob), _u8(sig_blob)
        tbs_off, sig_off = _u64(tbs_off), _u64(sig_off)
        ck = None if cert_key_id is None else _u64(cert_key_id)
        err = np.zeros(n, dtype=np.uint8)
        self.last_fenced = np.zeros(n, dtype=np.uint8)
        small = self.signature_verify_small(tbs_blob, tbs_off, sig_blob, sig_off, cert_key_id) if self._cross_check(n) else None
        self._check(self.lib.bftkv_gpu_signature_verify(self.h, n, _ptr(tbs_blob), _ptr(tbs_off), _ptr(sig_blob), _ptr(sig_off),
                                                        _ptr(ck), _ptr(err), _ptr(self.last_fenced)), "signature_verify")
        self._compare_small("signature_verify", small, err, self.last_fenced)
        return err

    def last_statuses(self):
        n = C.c_uint32(0)
        self._check(self.lib.bftkv_gpu_last_statuses(self.h, None, None, 0, C.byref(n)), "last_statuses")
        st = np.zeros(max(1, n.value), dtype=np.uint8)
        item = np.zeros(max(1, n.value), dtype=np.uint32)
        self._check(self.lib.bftkv_gpu_last_statuses(self.h, _ptr(st), _ptr(item), n.value, C.byref(n)), "last_statuses")
        return st[:n.value], item[:n.value]

    def last_counters(self):
        c = (C.c_uint64 * 4)()
        self._check(self.lib.bftkv_gpu_last_counters(self.h, c), "last_counters")
        return {"packets": c[0], "pubkey_ops": c[1], "items": c[2], "dsa_ops": c[3]}

    def last_sclk_mhz(self) -> float:
        v = C.c_float(0)
        self._check(self.lib.bftkv_gpu_last_sclk_mhz(self.h, C.byref(v)), "last_sclk_mhz")
        return float(v.value)

    PLAN_REPORT_SLOTS = (
        "words", "phase2_bound", "walk_fill", "mid_other", "mid_text",
        "wide1", "compare1", "compare1_3072", "compare1_4096", "dsa_mul1", "dsa_split1", "dsa_modexp1_4", "dsa_modexp1_8",
        "modexp2", "wide2", "modexp2_3072", "modexp2_4096", "compare2", "compare2_3072", "compare2_4096",
        "dsa_inv2_batched", "dsa_inv2", "dsa_mul2", "dsa_split2", "dsa_modexp2_4", "dsa_modexp2_8", "total")

    def last_plan_report(self):
        """Blocks per launch (0: not launched) of what the last resident big verify call enqueued behind its modexp
        (csrc/plan_report.h); raises NativeError when the last call was of another kind."""
        n = C.c_uint32(0)
        out = (C.c_uint32 * 64)()
        self._check(self.lib.bftkv_gpu_last_plan_report(self.h, out, 64, C.byref(n)), "last_plan_report")
        assert n.value == len(self.PLAN_REPORT_SLOTS), n.value
        return {k: int(out[i]) for i, k in enumerate(self.PLAN_REPORT_SLOTS)}

    def last_timing(self):
        ms = (C.c_float * 8)()
        self._check(self.lib.bftkv_gpu_last_timing(self.h, ms), "last_timing")
        return {"total": ms[0], "parse": ms[1], "hash": ms[2], "rsa": ms[3], "tally": ms[4], "compare": ms[5], "dsa": ms[6]}

    def signers(self, ss_blob, ss_off):
        n = len(ss_off) - 1
        ss_blob, ss_off = _u8(ss_blob), _u64(ss_off)
        cap = max(1, int(len(ss_blob) // 12) + 1)
        ids = np.zeros(cap, dtype=np.uint64)
        off = np.zeros(n + 1, dtype=np.uint64)
        self.last_fenced = np.zeros(n, dtype=np.uint8)
        self._check(self.lib.bftkv_gpu_signers_fenced(self.h, n, _ptr(ss_blob), _ptr(ss_off), _ptr(ids), _ptr(off), cap, _ptr(self.last_fenced)), "signers")
        return ids[:int(off[n])], off

    def quorum_tally(self, quorum: int, ids, list_off):
        n = len(list_off) - 1
        ids, list_off = _u64(ids), _u64(list_off)
        v = np.zeros(n, dtype=np.uint8)
        self._check(self.lib.bftkv_gpu_quorum_tally(self.h, quorum, n, _ptr(ids), _ptr(list_off), _ptr(v)), "quorum_tally")
        return v

    # ---- multi-GPU exchange step (RCCL)
    @staticmethod
    def comm_unique_id() -> np.ndarray:
        uid = np.zeros(128, dtype=np.uint8)
        rc = load_library().bftkv_gpu_comm_unique_id(_ptr(uid))
        if rc:
            raise NativeError("bftkv_gpu_comm_unique_id failed (%d): librccl not loadable" % rc)
        return uid

    def comm_init(self, n_ranks: int, rank: int, uid: np.ndarray):
        self._check(self.lib.bftkv_gpu_comm_init(self.h, n_ranks, rank, _ptr(np.ascontiguousarray(uid, dtype=np.uint8))), "comm_init")

    @staticmethod
    def comm_library():
        """(path of the librccl the library resolved, whether the process already held it)"""
        buf = C.create_string_buffer(1024)
        pre = C.c_int(0)
        rc = load_library().bftkv_gpu_comm_library(buf, 1024, C.byref(pre))
        if rc:
            raise NativeError("bftkv_gpu_comm_library failed (%d): librccl not loadable" % rc)
        return buf.value.decode(), bool(pre.value)

    def comm_selftest(self, nbytes: int = 4096):
        """Collective all-gather self-test on the verifier's stream; raises with the rank and RCCL's error string."""
        bad = C.c_uint32(0)
        self._check(self.lib.bftkv_gpu_comm_selftest(self.h, nbytes, C.byref(bad)), "comm_selftest")

    def allgather_verdicts(self, local_ptr: int, nbytes: int, out_ptr: int):
        self._check(self.lib.bftkv_gpu_allgather_verdicts(self.h, local_ptr, nbytes, out_ptr), "allgather_verdicts")

    def allgather_errs_dev(self, err_ptr: int, n_items: int, slots: int, out_ptr: int):
        """Asynchronous on the context's stream: pack err == 0 into a bitmap of ceil(slots/8) bytes, all-gather rank-major."""
        self._check(self.lib.bftkv_gpu_allgather_errs_dev(self.h, err_ptr, n_items, slots, out_ptr), "allgather_errs_dev")

    # ---- threshold share combine (config 5); numbers are Python ints at this level
    def modmul_product(self, factors, moduli, mod_idx, nbytes: int = 256):
        """factors: [n_ops][k] ints; returns [n_ops] ints = prod mod moduli[mod_idx[op]] (rsa.go:318-329)."""
        n, k = len(factors), len(factors[0])
        f = _ints_to_be([x for row in factors for x in row], nbytes)
        m = _ints_to_be(moduli, nbytes)
        mi = np.ascontiguousarray(mod_idx, dtype=np.uint32)
        out = np.zeros((n, nbytes), dtype=np.uint8)
        self._check(self.lib.bftkv_gpu_modmul_product(self.h, n, k, _ptr(f), nbytes, _ptr(mi), len(moduli), _ptr(m), _ptr(out)), "modmul_product")
        return [int.from_bytes(out[i].tobytes(), "big") for i in range(n)]

    def lagrange_combine(self, xs, ys, moduli, mod_idx, nbytes: int = 256):
        """xs: [n_ops][k] small ints, ys: [n_ops][k] ints -> ([n_ops] ints, status[n_ops]) (sss.go:69-107)."""
        n, k = len(xs), len(xs[0])
        x = np.ascontiguousarray(np.array(xs, dtype=np.int32))
        y = _ints_to_be([v for row in ys for v in row], nbytes)
        m = _ints_to_be(moduli, nbytes)
        mi = np.ascontiguousarray(mod_idx, dtype=np.uint32)
        out = np.zeros((n, nbytes), dtype=np.uint8)
        st = np.zeros(n + 8, dtype=np.uint8)
        self._check(self.lib.bftkv_gpu_lagrange_combine(self.h, n, k, _ptr(x), _ptr(y), nbytes, _ptr(mi), len(moduli), _ptr(m), _ptr(out),
                                                        _ptr(st)), "lagrange_combine")
        return [int.from_bytes(out[i].tobytes(), "big") for i in range(n)], st[:n]

    def dsa_calculate_r(self, xs, ri, vi, groups, group_idx, pbytes: int = 256, qbytes: int = 32):
        """CalculateR (dsa.go:33-52): xs/ri/vi [n_ops][k]; groups: list of (p, q) -> ([n_ops] ints, status)."""
        n, k = len(xs), len(xs[0])
        x = np.ascontiguousarray(np.array(xs, dtype=np.int32))
        r = _ints_to_be([v for row in ri for v in row], pbytes)
        v = _ints_to_be([v for row in vi for v in row], qbytes)
        p = _ints_to_be([g[0] for g in groups], pbytes)
        q = _ints_to_be([g[1] for g in groups], qbytes)
        gi = np.ascontiguousarray(group_idx, dtype=np.uint32)
        out = np.zeros((n, qbytes), dtype=np.uint8)
        st = np.zeros(n + 8, dtype=np.uint8)
        self._check(self.lib.bftkv_gpu_dsa_calculate_r(self.h, n, k, _ptr(x), _ptr(r), pbytes, _ptr(v), qbytes, _ptr(gi), len(groups), _ptr(p),
                                                       _ptr(q), _ptr(out), _ptr(st)), "dsa_calculate_r")
        return [int.from_bytes(out[i].tobytes(), "big") for i in range(n)], st[:n]

    def sss_distribute(self, polys, n_shares: int, moduli, mod_idx, nbytes: int = 256):
        """polys: [n_polys][k] ints (polys[p][0] = secret) -> [n_polys][n_shares] ints (sss.go:23-47)."""
        n, k = len(polys), len(polys[0])
        cf = _ints_to_be([c for row in polys for c in row], nbytes)
        m = _ints_to_be(moduli, nbytes)
        mi = np.ascontiguousarray(mod_idx, dtype=np.uint32)
        out = np.zeros((n * n_shares, nbytes), dtype=np.uint8)
        self._check(self.lib.bftkv_gpu_sss_distribute(self.h, n, n_shares, k, _ptr(cf), nbytes, _ptr(mi), len(moduli), _ptr(m), _ptr(out)),
                    "sss_distribute")
        return [[int.from_bytes(out[p * n_shares + x].tobytes(), "big") for x in range(n_shares)] for p in range(n)]

    def modinv(self, values, moduli, mod_idx, nbytes: int = 256):
        v = _ints_to_be(values, nbytes)
        m = _ints_to_be(moduli, nbytes)
        mi = np.ascontiguousarray(mod_idx, dtype=np.uint32)
        out = np.zeros((len(values), nbytes), dtype=np.uint8)
        st = np.zeros(len(values) + 8, dtype=np.uint8)
        self._check(self.lib.bftkv_gpu_modinv(self.h, len(values), _ptr(v), nbytes, _ptr(mi), len(moduli), _ptr(m), _ptr(out), _ptr(st)), "modinv")
        return [int.from_bytes(out[i].tobytes(), "big") for i in range(len(values))], st[:len(values)]

    def selftest_reduce(self, values, moduli, mod_idx, lanes: int, nbytes: int = 256):
        """values[i] - m when values[i] >= m else values[i] (values < 2m): the kernels' conditional subtraction on its own."""
        v = _ints_to_be(values, nbytes)
        m = _ints_to_be(moduli, nbytes)
        mi = np.ascontiguousarray(mod_idx, dtype=np.uint32)
        out = np.zeros((len(values), nbytes), dtype=np.uint8)
        self._check(self.lib.bftkv_gpu_selftest_reduce(self.h, len(values), _ptr(v), nbytes, _ptr(mi), len(moduli), _ptr(m), lanes, _ptr(out)),
                    "selftest_reduce")
        return [int.from_bytes(out[i].tobytes(), "big") for i in range(len(values))]

    def modexp_ops(self, base: np.ndarray, mod_idx: np.ndarray, mods: np.ndarray, exps: np.ndarray) -> np.ndarray:
        """out[i] = base[i] ^ exps[i] mod mods[mod_idx[i]] (one exponent per operation: CalculatePartialR, dsa.go:27-31)."""
        base, mods, exps = _u8(base), _u8(mods), _u8(exps)
        mod_idx = np.ascontiguousarray(mod_idx, dtype=np.uint32)
        assert exps.shape[0] == base.shape[0]
        out = np.zeros_like(base)
        self._check(self.lib.bftkv_gpu_modexp_ops(self.h, base.shape[0], _ptr(base), base.shape[1], _ptr(mod_idx), mods.shape[0],
                                                  _ptr(mods), _ptr(exps), exps.shape[1], _ptr(out)), "modexp_ops")
        return out

    def modexp(self, base: np.ndarray, mod_idx: np.ndarray, mods: np.ndarray, exps: np.ndarray) -> np.ndarray:
        """base [n, nbytes] u8 BE; mods [m, nbytes]; exps [m, exp_len] -> [n, nbytes]."""
        base, mods, exps = _u8(base), _u8(mods), _u8(exps)
        mod_idx = np.ascontiguousarray(mod_idx, dtype=np.uint32)
        out = np.zeros_like(base)
        self._check(self.lib.bftkv_gpu_modexp(self.h, base.shape[0], _ptr(base), base.shape[1], _ptr(mod_idx), mods.shape[0],
                                              _ptr(mods), _ptr(exps), exps.shape[1], _ptr(out)), "modexp")
        return out


    def ecdsa_calculate_r(self, xs, ri, vi, curve):
        """ECDSA CalculateR (ecdsa.go:36-59): xs [n_ops][k] ints, ri [n_ops][k] Marshal bytes (1 + 2 fbytes each), vi [n_ops][k]
        ints; curve: {p, n, b, gx, gy, bit_size} -> ([n_ops] ints, status)."""
        cb, bits, f = _curve_bytes(curve)
        n, k = len(xs), len(xs[0])
        x = np.ascontiguousarray(np.array(xs, dtype=np.int32))
        r = _u8(b"".join(bytes(v) for row in ri for v in row))
        v = _ints_to_be([v for row in vi for v in row], f)
        out = np.zeros((n, f), dtype=np.uint8)
        st = np.zeros(n + 8, dtype=np.uint8)
        self._check(self.lib.bftkv_gpu_ecdsa_calculate_r(self.h, n, k, _ptr(x), _ptr(r), _ptr(v), _ptr(cb), bits, _ptr(out), _ptr(st)),
                    "ecdsa_calculate_r")
        return [int.from_bytes(out[i].tobytes(), "big") for i in range(n)], st[:n]

    def ec_scalar_base_mult(self, scalars, curve):
        """ECDSA CalculatePartialR (ecdsa.go:31-34): [n_ops] ints -> ([n_ops] Marshal bytes, status)."""
        cb, bits, f = _curve_bytes(curve)
        n = len(scalars)
        sc = _ints_to_be(scalars, f)
        out = np.zeros((n, 1 + 2 * f), dtype=np.uint8)
        st = np.zeros(n + 8, dtype=np.uint8)
        self._check(self.lib.bftkv_gpu_ec_scalar_base_mult(self.h, n, _ptr(sc), f, _ptr(cb), bits, _ptr(out), _ptr(st)), "ec_scalar_base_mult")
        return [out[i].tobytes() for i in range(n)], st[:n]

    def _verdicts(self, label, shape, digests, sigs, slen, key_idx, call, ok=True):
        """The batched verdict call of every verify method: digests [n_ops] bytes of ONE length and sigs [n_ops] bytes of slen each
        (else ValueError "label: shape"), key_idx [n_ops] or None; call(n, dg, dlen, sg, ki, valid, st) -> rc, with ki a pointer or
        None and valid / st the result arrays -> (valid, status), uint8 each."""
        n = len(digests)
        dlen = len(digests[0]) if n else 1
        if any(len(d) != dlen for d in digests) or any(len(s) != slen for s in sigs) or not ok or len(sigs) != n:
            raise ValueError(label + ": " + shape)
        dg, sg = _u8(b"".join(bytes(d) for d in digests)), _u8(b"".join(bytes(s) for s in sigs))
        ki = None if key_idx is None else np.ascontiguousarray(key_idx, dtype=np.uint32)
        valid, st = np.zeros(n + 8, dtype=np.uint8), np.zeros(n + 8, dtype=np.uint8)
        self._check(call(n, _ptr(dg), dlen, _ptr(sg), None if ki is None else _ptr(ki), _ptr(valid), _ptr(st)), label)
        return valid[:n], st[:n]

    def ecdsa_verify(self, digests, sigs, keys, curve, key_idx=None):
        """crypto/ecdsa.Verify on raw signatures: digests [n_ops] bytes of ONE length (1..66), sigs [n_ops] bytes r || s (2 fbytes
        each), keys [n_keys] Marshal bytes (1 + 2 fbytes each), key_idx [n_ops] or None (key 0) -> (valid, status), uint8 each."""
        cb, bits, f = _curve_bytes(curve)
        kk = _u8(b"".join(bytes(k) for k in keys))
        return self._verdicts("ecdsa_verify", "digests of one length, sigs of 2 fbytes, keys of 1 + 2 fbytes", digests, sigs, 2 * f, key_idx,
                              lambda n, dg, dlen, sg, ki, valid, st: self.lib.bftkv_gpu_ecdsa_verify(
                                  self.h, n, dg, dlen, sg, ki, len(keys), _ptr(kk), _ptr(cb), bits, valid, st),
                              ok=all(len(k) == 1 + 2 * f for k in keys))

    def dsa_verify(self, digests, sigs, keys, groups, key_idx=None, pbytes=None, qbytes=None):
        """crypto/dsa.Verify on raw signatures: digests [n_ops] bytes of ONE length (1..64), sigs [n_ops] bytes r || s (2 qbytes each),
        groups [(p, q, g)] ints, keys [(group, y)], key_idx [n_ops] or None (key 0) -> (valid, status), uint8 each.  pbytes / qbytes
        default to the width of the widest p, g, y and to half a signature."""
        if qbytes is None:
            qbytes = len(sigs[0]) // 2 if len(digests) else max((int(g[1]).bit_length() + 7) // 8 for g in groups)
        if pbytes is None:
            pbytes = max(1, max((int(v).bit_length() + 7) // 8 for v in [g[0] for g in groups] + [g[2] for g in groups] + [k[1] for k in keys]))

        def call(n, dg, dlen, sg, ki, valid, st):
            p, q, g = (_ints_to_be([grp[i] for grp in groups], w) for i, w in ((0, pbytes), (1, qbytes), (2, pbytes)))
            y = _ints_to_be([k[1] for k in keys], pbytes)
            kg = np.ascontiguousarray([k[0] for k in keys], dtype=np.uint32)
            return self.lib.bftkv_gpu_dsa_verify(self.h, n, dg, dlen, sg, qbytes, ki, len(keys), _ptr(y), _ptr(kg), pbytes, len(groups), _ptr(p), _ptr(q),
                                                 _ptr(g), valid, st)
        return self._verdicts("dsa_verify", "digests of one length, sigs of 2 qbytes", digests, sigs, 2 * qbytes, key_idx, call)

    def ecdsa_keyset_create(self, keys, curve) -> int:
        """Register keys [n_keys] Marshal bytes (1 + 2 fbytes each) once: Unmarshal's checks and a table per key on the device.
        A refused key does not refuse the set (ecdsa_keyset_info counts it; its signatures are fenced)."""
        cb, bits, f = _curve_bytes(curve)
        if any(len(k) != 1 + 2 * f for k in keys):
            raise ValueError("ecdsa_keyset_create: keys of 1 + 2 fbytes")
        kk = _u8(b"".join(bytes(k) for k in keys))
        h = C.c_int(-1)
        self._check(self.lib.bftkv_gpu_ecdsa_keyset_create(self.h, len(keys), _ptr(kk), _ptr(cb), bits, C.byref(h)), "ecdsa_keyset_create")
        self._keyset_fbytes_cache()[h.value] = f
        return h.value

    def ecdsa_keyset_destroy(self, keyset: int):
        self._check(self.lib.bftkv_gpu_ecdsa_keyset_destroy(self.h, keyset), "ecdsa_keyset_destroy")
        self._keyset_fbytes_cache().pop(keyset, None)

    def ecdsa_keyset_info(self, keyset: int):
        """-> {n_keys, n_refused, window_bits, table_bytes}"""
        nk, nr, w, tb = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_uint64()
        self._check(self.lib.bftkv_gpu_ecdsa_keyset_info(self.h, keyset, C.byref(nk), C.byref(nr), C.byref(w), C.byref(tb)), "ecdsa_keyset_info")
        return {"n_keys": nk.value, "n_refused": nr.value, "window_bits": w.value, "table_bytes": tb.value}

    def _keyset_fbytes_cache(self):
        """handle -> coordinate length of the set's curve; one dictionary on the root, which its forks share"""
        ctx = self
        while getattr(ctx, "root", None) is not None:
            ctx = ctx.root
        return ctx.__dict__.setdefault("_keyset_fbytes", {})

    def _ecdsa_keyset_fbytes(self, keyset: int) -> int:
        """The coordinate length of a set's curve, as ecdsa_keyset_create recorded it.  A handle that was made through the C entry
        itself is looked up once, from the size of its tables (windows x 2 L x 2^w words per key); ecdsa_keyset_destroy forgets it."""
        cache = self._keyset_fbytes_cache()
        if keyset not in cache:
            info = self.ecdsa_keyset_info(keyset)
            w, words = info["window_bits"], info["table_bytes"] // (4 * info["n_keys"])
            cache[keyset] = next(f for f, nw in ((28, 7), (32, 8), (48, 12), (66, 17)) if (((8 * f + w - 1) // w * 2 * nw) << w) == words)
        return cache[keyset]

    def ecdsa_verify_keyset(self, keyset: int, digests, sigs, key_idx=None):
        """ecdsa_verify under the keys of a set: digests [n_ops] bytes of ONE length, sigs [n_ops] bytes r || s of the set's curve,
        key_idx [n_ops] into the set or None (key 0) -> (valid, status), uint8 each."""
        return self._verdicts("ecdsa_verify_keyset", "digests of one length, sigs of 2 fbytes", digests, sigs, 2 * self._ecdsa_keyset_fbytes(keyset), key_idx,
                              lambda n, dg, dlen, sg, ki, valid, st: self.lib.bftkv_gpu_ecdsa_verify_keyset(self.h, keyset, n, dg, dlen, sg, ki, valid, st))

    def selftest_ecdsa_keyset_table(self, keyset: int, key: int) -> np.ndarray:
        """One key's table as the device built it (uint32 words, the layout of ec_field.h fb_table_build)."""
        info = self.ecdsa_keyset_info(keyset)
        words = np.zeros(info["table_bytes"] // (4 * info["n_keys"]), dtype=np.uint32)
        self._check(self.lib.bftkv_gpu_selftest_ecdsa_keyset_table(self.h, keyset, key, words.ctypes.data, len(words)), "selftest_ecdsa_keyset_table")
        return words

    def dsa_keyset_create(self, keys, groups, window_bits=0, pbytes=None, qbytes=None) -> int:
        """Register groups [(p, q, g)] ints and keys [(group, y)] once: the Montgomery rows and a fixed-base window table per g and
        y on the device.  window_bits 4 .. 16, 0 for the default of 8; pbytes / qbytes default to the width of the widest p, g, y
        and of the widest q."""
        if qbytes is None:
            qbytes = max(1, max((int(g[1]).bit_length() + 7) // 8 for g in groups))
        if pbytes is None:
            pbytes = max(1, max((int(v).bit_length() + 7) // 8 for v in [g[0] for g in groups] + [g[2] for g in groups] + [k[1] for k in keys]))
        p, q, g = (_ints_to_be([grp[i] for grp in groups], w) for i, w in ((0, pbytes), (1, qbytes), (2, pbytes)))
        y = _ints_to_be([k[1] for k in keys], pbytes)
        kg = np.ascontiguousarray([k[0] for k in keys], dtype=np.uint32)
        h = C.c_int(-1)
        self._check(self.lib.bftkv_gpu_dsa_keyset_create(self.h, len(keys), _ptr(y), _ptr(kg), pbytes, len(groups), _ptr(p), _ptr(q), _ptr(g), qbytes,
                                                         window_bits, C.byref(h)), "dsa_keyset_create")
        return h.value

    def dsa_keyset_destroy(self, keyset: int):
        self._check(self.lib.bftkv_gpu_dsa_keyset_destroy(self.h, keyset), "dsa_keyset_destroy")

    def dsa_keyset_info(self, keyset: int):
        """-> {n_keys, n_groups, pbytes, qbytes, window_bits, windows, table_bytes}"""
        v = [C.c_uint32() for _ in range(6)]
        tb = C.c_uint64()
        self._check(self.lib.bftkv_gpu_dsa_keyset_info(self.h, keyset, *[C.byref(x) for x in v], C.byref(tb)), "dsa_keyset_info")
        names = ("n_keys", "n_groups", "pbytes", "qbytes", "window_bits", "windows")
        return dict(zip(names, (x.value for x in v)), table_bytes=tb.value)

    def dsa_verify_keyset(self, keyset: int, digests, sigs, key_idx=None):
        """dsa_verify under the keys of a set: digests [n_ops] bytes of ONE length (1..64), sigs [n_ops] bytes r || s (2 qbytes of
        the set), key_idx [n_ops] into the set or None (key 0) -> (valid, status), uint8 each."""
        return self._verdicts("dsa_verify_keyset", "digests of one length, sigs of 2 qbytes", digests, sigs, 2 * self.dsa_keyset_info(keyset)["qbytes"], key_idx,
                              lambda n, dg, dlen, sg, ki, valid, st: self.lib.bftkv_gpu_dsa_verify_keyset(self.h, keyset, n, dg, dlen, sg, ki, valid, st))

    def selftest_dsa_keyset_table(self, keyset: int, base: int) -> np.ndarray:
        """One base's table as the device built it (the groups' g first, then the keys' y): uint32 [windows][2^w - 1][76]."""
        info = self.dsa_keyset_info(keyset)
        nent = (1 << info["window_bits"]) - 1
        words = np.zeros(info["windows"] * nent * 76, dtype=np.uint32)
        self._check(self.lib.bftkv_gpu_selftest_dsa_keyset_table(self.h, keyset, base, words.ctypes.data, len(words)), "selftest_dsa_keyset_table")
        return words.reshape(info["windows"], nent, 76)

    def rsa_verify(self, digests, sigs, keys, hash_id: int, key_idx=None, nbytes=None):
        """rsa.VerifyPKCS1v15 on raw signatures: digests [n_ops] bytes of ONE length (the size of hash_id's hash; 1..64 for hash_id
        0, no prefix), sigs [n_ops] bytes of nbytes each, keys [(n, e)] ints, key_idx [n_ops] or None (key 0) -> (valid, status),
        uint8 each.  nbytes defaults to the length of a signature, or to the widest modulus."""
        if nbytes is None:
            nbytes = len(sigs[0]) if len(digests) else max(1, max((int(k[0]).bit_length() + 7) // 8 for k in keys))

        def call(n, dg, dlen, sg, ki, valid, st):
            kn = _ints_to_be([k[0] for k in keys], nbytes)
            ke = np.ascontiguousarray([k[1] for k in keys], dtype=np.uint32)
            return self.lib.bftkv_gpu_rsa_verify(self.h, n, dg, hash_id, dlen, sg, nbytes, ki, len(keys), _ptr(kn), _ptr(ke), valid, st)
        return self._verdicts("rsa_verify", "digests of one length, sigs of nbytes", digests, sigs, nbytes, key_idx, call)

    def rsa_keyset_create(self, keys, nbytes=None) -> int:
        """Register keys [(n, e)] ints once: their Montgomery rows stay on the device.  An even modulus does not refuse the set
        (rsa_keyset_info counts it; its signatures are fenced, or refused by the length rule).  nbytes defaults to the widest modulus."""
        if nbytes is None:
            nbytes = max(1, max((int(k[0]).bit_length() + 7) // 8 for k in keys))
        kn = _ints_to_be([k[0] for k in keys], nbytes)
        ke = np.ascontiguousarray([k[1] for k in keys], dtype=np.uint32)
        h = C.c_int(-1)
        self._check(self.lib.bftkv_gpu_rsa_keyset_create(self.h, len(keys), _ptr(kn), _ptr(ke), nbytes, C.byref(h)), "rsa_keyset_create")
        return h.value

    def rsa_keyset_destroy(self, keyset: int):
        self._check(self.lib.bftkv_gpu_rsa_keyset_destroy(self.h, keyset), "rsa_keyset_destroy")

    def rsa_keyset_info(self, keyset: int):
        """-> {n_keys, n_refused, nbytes}"""
        v = [C.c_uint32() for _ in range(3)]
        self._check(self.lib.bftkv_gpu_rsa_keyset_info(self.h, keyset, *[C.byref(x) for x in v]), "rsa_keyset_info")
        return dict(zip(("n_keys", "n_refused", "nbytes"), (x.value for x in v)))

    def rsa_verify_keyset(self, keyset: int, digests, sigs, hash_id: int, key_idx=None):
        """rsa_verify under the keys of a set: digests [n_ops] bytes of ONE length, sigs [n_ops] bytes of the set's nbytes, key_idx
        [n_ops] into the set or None (key 0) -> (valid, status), uint8 each."""
        return self._verdicts("rsa_verify_keyset", "digests of one length, sigs of the set's nbytes", digests, sigs, self.rsa_keyset_info(keyset)["nbytes"], key_idx,
                              lambda n, dg, dlen, sg, ki, valid, st: self.lib.bftkv_gpu_rsa_verify_keyset(self.h, keyset, n, dg, hash_id, dlen, sg, ki, valid, st))

    # ---- raw RSA signing under resident private key sets (rsa.SignPKCS1v15)
    def rsa_signer_create(self, keys, nbytes=None, pbytes=None) -> int:
        """Register private keys, dicts of ints {n, e, p, q, dp, dq, qinv}: their rows stay on the device.  A key with an even n, or
        with p or q even or below 3, does not refuse the set (rsa_signer_info counts it; its signatures are fenced).  nbytes and pbytes
        default to the widest modulus and the widest of the private parts."""
        if nbytes is None:
            nbytes = max(1, max((int(k["n"]).bit_length() + 7) // 8 for k in keys))
        if pbytes is None:
            pbytes = max(1, max((int(k[f]).bit_length() + 7) // 8 for k in keys for f in ("p", "q", "dp", "dq", "qinv")))
        kn = _ints_to_be([k["n"] for k in keys], nbytes)
        ke = np.ascontiguousarray([k["e"] for k in keys], dtype=np.uint32)
        parts = [_ints_to_be([k[f] for k in keys], pbytes) for f in ("p", "q", "dp", "dq", "qinv")]
        h = C.c_int(-1)
        self._check(self.lib.bftkv_gpu_rsa_signer_create(self.h, len(keys), _ptr(kn), _ptr(ke), nbytes, *[_ptr(a) for a in parts], pbytes, C.byref(h)),
                    "rsa_signer_create")
        return h.value

    def rsa_signer_destroy(self, signer: int):
        self._check(self.lib.bftkv_gpu_rsa_signer_destroy(self.h, signer), "rsa_signer_destroy")

    def rsa_signer_info(self, signer: int):
        """-> {n_keys, n_refused, nbytes, pbytes}"""
        v = [C.c_uint32() for _ in range(4)]
        self._check(self.lib.bftkv_gpu_rsa_signer_info(self.h, signer, *[C.byref(x) for x in v]), "rsa_signer_info")
        return dict(zip(("n_keys", "n_refused", "nbytes", "pbytes"), (x.value for x in v)))

    def rsa_sign_keyset(self, signer: int, digests, hash_id: int, key_idx=None):
        """rsa.SignPKCS1v15 on raw digests under the keys of a signer set: digests [n_ops] bytes of ONE length (the size of hash_id's
        hash; 1..64 for hash_id 0), key_idx [n_ops] into the set or None (key 0) -> (sigs [n_ops, nbytes], status [n_ops]), uint8."""
        n = len(digests)
        dlen = len(digests[0]) if n else 0
        if any(len(d) != dlen for d in digests):
            raise ValueError("rsa_sign_keyset: digests of one length")
        dg = np.frombuffer(b"".join(bytes(d) for d in digests), dtype=np.uint8).copy() if n else np.zeros(1, dtype=np.uint8)
        ki = None if key_idx is None else np.ascontiguousarray(key_idx, dtype=np.uint32)
        assert ki is None or len(ki) == n
        nbytes = self.rsa_signer_info(signer)["nbytes"]
        sig, st = np.zeros((n, nbytes), dtype=np.uint8), np.zeros(n, dtype=np.uint8)
        self._check(self.lib.bftkv_gpu_rsa_sign_keyset(self.h, signer, n, _ptr(dg), hash_id, dlen, None if ki is None else ki.ctypes.data, _ptr(sig),
                                                       _ptr(st)), "rsa_sign_keyset")
        return sig, st

    def selftest_rsa_crt(self, signer: int, values, key_idx=None):
        """The chains and the recombination on values [n_ops] ints below 2^(8 nbytes), without padding and without the check
        -> (out [n_ops, nbytes], status [n_ops])."""
        nbytes = self.rsa_signer_info(signer)["nbytes"]
        n = len(values)
        cv = _ints_to_be(list(values), nbytes) if n else np.zeros((1, nbytes), dtype=np.uint8)
        ki = None if key_idx is None else np.ascontiguousarray(key_idx, dtype=np.uint32)
        assert ki is None or len(ki) == n
        out, st = np.zeros((n, nbytes), dtype=np.uint8), np.zeros(n, dtype=np.uint8)
        self._check(self.lib.bftkv_gpu_selftest_rsa_crt(self.h, signer, n, _ptr(cv), None if ki is None else ki.ctypes.data, _ptr(out), _ptr(st)),
                    "selftest_rsa_crt")
        return out, st

    # ---- threshold password authentication (crypto/auth): rows of uint8, big-endian
    def tpa_yi(self, x, y, mods, mod_idx=None):
        """makeYi: yi[i] = x[i] ^ y[i] mod mods[mod_idx[i]].  x [n, nbytes], y [n, exp_len], mods [m, nbytes], mod_idx [n] or None
        (modulus 0) -> (yi [n, nbytes], status [n])."""
        x, y, mods = _u8(x), _u8(y), _u8(mods)
        mi = None if mod_idx is None else np.ascontiguousarray(mod_idx, dtype=np.uint32)
        assert y.shape[0] == x.shape[0]
        out, st = np.zeros_like(x), np.zeros(x.shape[0], dtype=np.uint8)
        rc = self.lib.bftkv_gpu_tpa_yi(self.h, x.shape[0], _ptr(x), x.shape[1], _ptr(y), y.shape[1], None if mi is None else mi.ctypes.data,
                                       mods.shape[0], _ptr(mods), _ptr(out), _ptr(st))
        self._check(rc, "tpa_yi")
        return out, st

    def _tpa_kdf(self, what, call, base, xi, xi_len, exps, salt, mods, mod_idx):
        base, xi, exps, mods = _u8(base), _u8(xi), _u8(exps), _u8(mods)
        n, nbytes = base.shape
        salt = None if salt is None or np.size(salt) == 0 else _u8(salt).reshape(n, -1)
        salt_len = 0 if salt is None else salt.shape[1]
        xl = np.ascontiguousarray(xi_len, dtype=np.uint32)
        mi = None if mod_idx is None else np.ascontiguousarray(mod_idx, dtype=np.uint32)
        assert xi.shape == base.shape and exps.shape[0] == n and len(xl) == n
        keys, mac, st = np.zeros((n, 32), dtype=np.uint8), np.zeros((n, 32), dtype=np.uint8), np.zeros(n, dtype=np.uint8)
        rc, res = call(n, _ptr(base), _ptr(xi), xl.ctypes.data, nbytes, _ptr(exps), exps.shape[1], _ptr(salt), salt_len,
                       None if mi is None else mi.ctypes.data, mods.shape[0], _ptr(mods), _ptr(keys), _ptr(mac), _ptr(st))
        self._check(rc, what)
        return res + (keys, mac, st)

    def tpa_bi(self, v, xi, xi_len, b, salt, mods, mod_idx=None):
        """makeBi: bi = v ^ b, ki = SetBytes(xi[:xi_len]) ^ b, keys = km | ke of keySched(ki.Bytes(), salt), mac = HMAC(km, xi | bi.Bytes()).
        v, xi [n, nbytes], xi_len [n], b [n, exp_len], salt [n, salt_len] or None -> (bi [n, nbytes], keys [n, 32], mac [n, 32], status)."""
        def call(n, pv, pxi, pxl, nbytes, pb, el, ps, sl, pmi, nm, pm, pk, pmac, pst):
            out = np.zeros((n, nbytes), dtype=np.uint8)
            return self.lib.bftkv_gpu_tpa_bi(self.h, n, pv, pxi, pxl, nbytes, pb, el, ps, sl, pmi, nm, pm, _ptr(out), pk, pmac, pst), (out,)
        return self._tpa_kdf("tpa_bi", call, v, xi, xi_len, b, salt, mods, mod_idx)

    def tpa_ni(self, bi, xi, xi_len, e, salt, mods, mod_idx=None):
        """processBi: ki = bi ^ e, the same keySched, ni = HMAC(km, xi | bi.Bytes()) over the bytes of bi as given
        -> (keys [n, 32], ni [n, 32], status)."""
        def call(n, pbi, pxi, pxl, nbytes, pe, el, ps, sl, pmi, nm, pm, pk, pmac, pst):
            return self.lib.bftkv_gpu_tpa_ni(self.h, n, pbi, pxi, pxl, nbytes, pe, el, ps, sl, pmi, nm, pm, pk, pmac, pst), ()
        return self._tpa_kdf("tpa_ni", call, bi, xi, xi_len, e, salt, mods, mod_idx)

    # ---- threshold RSA signing, the server's side (rsaContext.Sign): rows of uint8, big-endian
    def rsa_partial_sign(self, t, t_len, mods, exps, sign, mod_idx=None, frag_req=None, exp_used=None):
        """The partial signatures of a batch of sign requests.  t [n_reqs, t_cap] with t_len [n_reqs] bytes at the front of each row,
        mods [m, nbytes], mod_idx [n_reqs] or None (modulus 0); exps [n_frags, exp_len] right-aligned magnitudes, sign [n_frags] the stored
        bytes, frag_req [n_frags] or None (request 0), exp_used [n_frags] or None (exp_len) -> (out [n_frags, nbytes], status [n_frags])."""
        t, mods, exps, sign = _u8(t), _u8(mods), _u8(exps), _u8(sign)
        tl = np.ascontiguousarray(t_len, dtype=np.uint32)
        n_reqs, n_frags, nbytes = len(tl), exps.shape[0], mods.shape[1]
        t = t.reshape(n_reqs, t.size // max(n_reqs, 1))
        opt = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.uint32)      # noqa: E731
        mi, fr, eu = opt(mod_idx), opt(frag_req), opt(exp_used)
        assert len(sign) == n_frags and all(a is None or len(a) == n for a, n in ((mi, n_reqs), (fr, n_frags), (eu, n_frags)))
        addr = lambda a: None if a is None else a.ctypes.data      # noqa: E731
        out, st = np.zeros((n_frags, nbytes), dtype=np.uint8), np.zeros(n_frags, dtype=np.uint8)
        rc = self.lib.bftkv_gpu_rsa_partial_sign(self.h, n_reqs, _ptr(t) if t.shape[1] else None, t.shape[1], tl.ctypes.data, addr(mi), mods.shape[0],
                                                 _ptr(mods), nbytes, n_frags, addr(fr), _ptr(exps), exps.shape[1], addr(eu), _ptr(sign), _ptr(out), _ptr(st))
        self._check(rc, "rsa_partial_sign")
        return out, st

    # ---- threshold DSA / ECDSA signing, the server's side (dsaContext.Sign): rows of uint8, big-endian
    def tdsa_share(self, keyset: int, shares, group_idx=None):
        """Phase 2 under a resident DSA key set: shares [n_reqs, m, 4, qbytes] (k, a, b, c of every share), group_idx [n_reqs] or None
        (group 0) -> (ri [n_reqs, pbytes], vi, ki, ci [n_reqs, qbytes], status [n_reqs])."""
        info = self.dsa_keyset_info(keyset)
        sh = _u8(shares)
        n, m = sh.shape[0], sh.shape[1]
        assert sh.shape[2:] == (4, info["qbytes"])
        gi = None if group_idx is None else np.ascontiguousarray(group_idx, dtype=np.uint32)
        assert gi is None or len(gi) == n
        ri = np.zeros((n, info["pbytes"]), dtype=np.uint8)
        vi, ki, ci = (np.zeros((n, info["qbytes"]), dtype=np.uint8) for _ in range(3))
        st = np.zeros(n, dtype=np.uint8)
        self._check(self.lib.bftkv_gpu_tdsa_share(self.h, keyset, n, None if gi is None else gi.ctypes.data, m, _ptr(sh), _ptr(ri), _ptr(vi), _ptr(ki),
                                                  _ptr(ci), _ptr(st)), "tdsa_share")
        return ri, vi, ki, ci, st

    def tecdsa_share(self, shares, curve):
        """Phase 2 on a recognised curve: shares [n_reqs, m, 4, fbytes] -> (ri [n_reqs, 1 + 2 fbytes], vi, ki, ci [n_reqs, fbytes], status)."""
        cb, bits, f = _curve_bytes(curve)
        sh = _u8(shares)
        n, m = sh.shape[0], sh.shape[1]
        assert sh.shape[2:] == (4, f)
        ri = np.zeros((n, 1 + 2 * f), dtype=np.uint8)
        vi, ki, ci = (np.zeros((n, f), dtype=np.uint8) for _ in range(3))
        st = np.zeros(n, dtype=np.uint8)
        self._check(self.lib.bftkv_gpu_tecdsa_share(self.h, n, m, _ptr(sh), _ptr(cb), bits, _ptr(ri), _ptr(vi), _ptr(ki), _ptr(ci), _ptr(st)), "tecdsa_share")
        return ri, vi, ki, ci, st

    def tsig_partial_s(self, m_in, r, y, k, c, q, mod_idx=None):
        """Phase 3 for both schemes: m_in, r, y, k, c [n_reqs, nbytes], q [n_mods, nbytes], mod_idx [n_reqs] or None (modulus 0)
        -> (si [n_reqs, nbytes], status [n_reqs])."""
        mm, rr, yy, kk, cc, qq = (_u8(a) for a in (m_in, r, y, k, c, q))
        n, nbytes = rr.shape
        assert all(a.shape == (n, nbytes) for a in (mm, yy, kk, cc)) and qq.shape[1] == nbytes
        mi = None if mod_idx is None else np.ascontiguousarray(mod_idx, dtype=np.uint32)
        si, st = np.zeros((n, nbytes), dtype=np.uint8), np.zeros(n, dtype=np.uint8)
        self._check(self.lib.bftkv_gpu_tsig_partial_s(self.h, n, _ptr(mm), _ptr(rr), _ptr(yy), _ptr(kk), _ptr(cc), nbytes,
                                                      None if mi is None else mi.ctypes.data, qq.shape[0], _ptr(qq), _ptr(si), _ptr(st)), "tsig_partial_s")
        return si, st


class Batcher:
    """bftkv_gpu_batcher: blocking one-message calls from many threads, aggregated into device batches."""

    def __init__(self, ctx: Context, max_items: int = 256, max_wait_us: int = 200, n_lanes: int = 0):
        self.ctx = ctx
        self.lib = ctx.lib
        self.h = C.c_void_p(self.lib.bftkv_gpu_batcher_create_lanes(ctx.h, max_items, max_wait_us, n_lanes))
        if not self.h:
            raise NativeError("bftkv_gpu_batcher_create_lanes failed")

    def close(self):
        if self.h:
            self.lib.bftkv_gpu_batcher_destroy(self.h)
            self.h = None

    def collective_verify(self, quorum: int, tbs: bytes, ss: bytes, raw: bool = False):
        """raw=True returns (rc, err, fenced) without raising (the fail-closed tests look at err when rc != 0)."""
        err = np.zeros(1, dtype=np.uint8)
        fenced = np.zeros(1, dtype=np.uint8)
        rc = self.lib.bftkv_gpu_batcher_collective_verify(self.h, quorum, tbs, len(tbs), ss, len(ss), _ptr(err), _ptr(fenced))
        if raw:
            return rc, int(err[0]), int(fenced[0])
        if rc:
            raise NativeError("batcher collective_verify failed: %d" % rc)
        return int(err[0])

    def signature_verify(self, tbs: bytes, sig: bytes, cert_key_id: Optional[int] = None, raw: bool = False):
        err = np.zeros(1, dtype=np.uint8)
        ck = None if cert_key_id is None else np.array([cert_key_id], dtype=np.uint64)
        fenced = np.zeros(1, dtype=np.uint8)
        rc = self.lib.bftkv_gpu_batcher_signature_verify(self.h, tbs, len(tbs), sig, len(sig), _ptr(ck), _ptr(err), _ptr(fenced))
        if raw:
            return rc, int(err[0]), int(fenced[0])
        if rc:
            raise NativeError("batcher signature_verify failed: %d" % rc)
        return int(err[0])

    def cert_verify(self, cert: bytes, tbs: bytes, sig: Optional[bytes], raw: bool = False):
        """bftkv_gpu_batcher_cert_verify: Signature.Issuer(sig) + VerifyWithCertificate(tbs, sig, issuer) for a principal outside the
        node keyring; sig=None asks for the issuer alone.  Returns (err, fenced, issuer_key_id, fingerprint)."""
        err = np.zeros(1, dtype=np.uint8)
        fenced = np.zeros(1, dtype=np.uint8)
        iid = np.zeros(1, dtype=np.uint64)
        fp = np.zeros(20, dtype=np.uint8)
        rc = self.lib.bftkv_gpu_batcher_cert_verify(self.h, cert, len(cert), tbs, len(tbs), sig, 0 if sig is None else len(sig), _ptr(err), _ptr(fenced),
                                                    iid.ctypes.data, _ptr(fp))
        if raw:
            return rc, int(err[0]), int(fenced[0])
        if rc:
            raise NativeError("batcher cert_verify failed: %d" % rc)
        return int(err[0]), int(fenced[0]), int(iid[0]), fp.tobytes()

    def cert_entity(self, cert: bytes, cap: int = 256):
        """bftkv_gpu_batcher_cert_entity: Issuer(sig) without ReadEntity on the CPU.  Returns (rc, err, fenced, issuer_key_id,
        fingerprint, entity_off, entity_len, roles) with roles = [(role number, index, chosen)]."""
        err, fenced = np.zeros(1, dtype=np.uint8), np.zeros(1, dtype=np.uint8)
        iid, rng = np.zeros(1, dtype=np.uint64), np.zeros(2, dtype=np.uint64)
        fp = np.zeros(20, dtype=np.uint8)
        while True:
            roles, n = np.zeros(max(1, cap), dtype=np.uint32), np.zeros(1, dtype=np.uint32)
            rc = self.lib.bftkv_gpu_batcher_cert_entity(self.h, cert, len(cert), _ptr(err), _ptr(fenced), iid.ctypes.data, _ptr(fp), rng.ctypes.data,
                                                        rng.ctypes.data + 8, roles.ctypes.data, cap, n.ctypes.data)
            if rc == -3 and int(n[0]) > cap:
                cap = int(n[0])
                continue
            return rc, int(err[0]), int(fenced[0]), int(iid[0]), fp.tobytes(), int(rng[0]), int(rng[1]), [(int(r) & 0xFF, (int(r) >> 8) & 0xFFFF, bool(int(r) >> 24)) for r in roles[:int(n[0])]]

    def message_verify(self, msg: bytes):
        """One transport message through the batcher: (status, signer_key_id, peer_id, plain, file_name)."""
        st = np.zeros(1, dtype=np.uint8)
        ids = np.zeros(2, dtype=np.uint64)
        plain = np.zeros(max(1, len(msg)), dtype=np.uint8)
        plen = np.zeros(1, dtype=np.uint64)
        fn = np.zeros(256, dtype=np.uint8)
        fl = np.zeros(1, dtype=np.uint8)
        rc = self.lib.bftkv_gpu_batcher_message_verify(self.h, msg, len(msg), _ptr(st), ids.ctypes.data, ids.ctypes.data + 8, _ptr(plain),
                                                       len(plain), _ptr(plen), _ptr(fn), _ptr(fl))
        if rc:
            raise NativeError("batcher message_verify failed: %d" % rc)
        return int(st[0]), int(ids[0]), int(ids[1]), plain[:int(plen[0])].tobytes(), fn[:int(fl[0])].tobytes()

    # ---- one threshold share-combine operation per call (numbers are Python ints; returns (rc, status, value))
    def modmul_product(self, factors, mod: int, nbytes: int = 256):
        """prod factors mod `mod` (calculateSignature, rsa.go:318-329) as ONE micro-batched operation."""
        f, m = _ints_to_be(factors, nbytes), _ints_to_be([mod], nbytes)
        out, st = np.full(nbytes, 0xAA, dtype=np.uint8), np.zeros(1, dtype=np.uint8)
        rc = self.lib.bftkv_gpu_batcher_modmul_product(self.h, len(factors), _ptr(f), nbytes, _ptr(m), _ptr(out), _ptr(st))
        return rc, int(st[0]), int.from_bytes(out.tobytes(), "big")

    def lagrange_combine(self, xs, ys, mod: int, nbytes: int = 256):
        """sum Lagrange(x_j) y_j mod `mod` (calculateSecret sss.go:81-92, calculateS dsa_core.go:389-403)."""
        x = np.ascontiguousarray(np.array(xs, dtype=np.int32))
        y, m = _ints_to_be(ys, nbytes), _ints_to_be([mod], nbytes)
        out, st = np.full(nbytes, 0xAA, dtype=np.uint8), np.zeros(1, dtype=np.uint8)
        rc = self.lib.bftkv_gpu_batcher_lagrange_combine(self.h, len(xs), _ptr(x), _ptr(y), nbytes, _ptr(m), _ptr(out), _ptr(st))
        return rc, int(st[0]), int.from_bytes(out.tobytes(), "big")

    def dsa_calculate_r(self, xs, ri, vi, p: int, q: int, pbytes: int = 256, qbytes: int = 32):
        """CalculateR (dsa.go:33-52)."""
        x = np.ascontiguousarray(np.array(xs, dtype=np.int32))
        r, v = _ints_to_be(ri, pbytes), _ints_to_be(vi, qbytes)
        pb, qb = _ints_to_be([p], pbytes), _ints_to_be([q], qbytes)
        out, st = np.full(qbytes, 0xAA, dtype=np.uint8), np.zeros(1, dtype=np.uint8)
        rc = self.lib.bftkv_gpu_batcher_dsa_calculate_r(self.h, len(xs), _ptr(x), _ptr(r), pbytes, _ptr(v), qbytes, _ptr(pb), _ptr(qb), _ptr(out), _ptr(st))
        return rc, int(st[0]), int.from_bytes(out.tobytes(), "big")

    def ecdsa_calculate_r(self, xs, ri, vi, curve):
        """ECDSA CalculateR (ecdsa.go:36-59) for one operation: ri [k] Marshal bytes, vi [k] ints -> (rc, status, r)."""
        cb, bits, f = _curve_bytes(curve)
        x = np.ascontiguousarray(np.array(xs, dtype=np.int32))
        r, v = _u8(b"".join(bytes(p) for p in ri)), _ints_to_be(vi, f)
        out, st = np.full(f, 0xAA, dtype=np.uint8), np.zeros(1, dtype=np.uint8)
        rc = self.lib.bftkv_gpu_batcher_ecdsa_calculate_r(self.h, len(xs), _ptr(x), _ptr(r), _ptr(v), _ptr(cb), bits, _ptr(out), _ptr(st))
        return rc, int(st[0]), int.from_bytes(out.tobytes(), "big")

    def ecdsa_verify(self, digest: bytes, sig: bytes, key: bytes, curve):
        """crypto/ecdsa.Verify for one raw signature r || s under Marshal bytes `key` -> (rc, status, valid)."""
        cb, bits, f = _curve_bytes(curve)
        if len(sig) != 2 * f or len(key) != 1 + 2 * f or not digest:
            raise ValueError("ecdsa_verify: sig of 2 fbytes, key of 1 + 2 fbytes, a non-empty digest")
        dg, sg, kk = _u8(digest), _u8(sig), _u8(key)
        valid, st = np.full(1, 0xAA, dtype=np.uint8), np.zeros(1, dtype=np.uint8)
        rc = self.lib.bftkv_gpu_batcher_ecdsa_verify(self.h, _ptr(dg), len(digest), _ptr(sg), _ptr(kk), _ptr(cb), bits, _ptr(valid), _ptr(st))
        return rc, int(st[0]), int(valid[0])

    def dsa_verify(self, digest: bytes, sig: bytes, group, y: int, pbytes=None):
        """crypto/dsa.Verify for one raw signature r || s (2 qbytes) under group (p, q, g) and public value y -> (rc, status, valid)."""
        qbytes = len(sig) // 2
        if pbytes is None:
            pbytes = max(1, max((int(v).bit_length() + 7) // 8 for v in (group[0], group[2], y)))
        if not digest or not sig or len(sig) != 2 * qbytes:
            raise ValueError("dsa_verify: sig of 2 qbytes, a non-empty digest")
        dg, sg = _u8(digest), _u8(sig)
        p, g, yy = (_ints_to_be([v], pbytes) for v in (group[0], group[2], y))
        q = _ints_to_be([group[1]], qbytes)
        valid, st = np.full(1, 0xAA, dtype=np.uint8), np.zeros(1, dtype=np.uint8)
        rc = self.lib.bftkv_gpu_batcher_dsa_verify(self.h, _ptr(dg), len(digest), _ptr(sg), qbytes, _ptr(yy), pbytes, _ptr(p), _ptr(q), _ptr(g),
                                                   _ptr(valid), _ptr(st))
        return rc, int(st[0]), int(valid[0])

    def _verdict(self, digest: bytes, sig: bytes, call):
        """One signature against a resident key set: call(dg, dlen, sg, valid, st) -> rc; -> (rc, status, valid)."""
        dg, sg = _u8(digest), _u8(sig)
        valid, st = np.full(1, 0xAA, dtype=np.uint8), np.zeros(1, dtype=np.uint8)
        rc = call(_ptr(dg), len(digest), _ptr(sg), _ptr(valid), _ptr(st))
        return rc, int(st[0]), int(valid[0])

    def ecdsa_verify_keyset(self, keyset: int, key: int, digest: bytes, sig: bytes):
        """crypto/ecdsa.Verify for one raw signature r || s under key `key` of a resident key set -> (rc, status, valid)."""
        if not digest or len(sig) != 2 * self.ctx._ecdsa_keyset_fbytes(keyset):
            raise ValueError("ecdsa_verify_keyset: sig of 2 fbytes of the set's curve, a non-empty digest")
        return self._verdict(digest, sig, lambda dg, dlen, sg, valid, st: self.lib.bftkv_gpu_batcher_ecdsa_verify_keyset(
            self.h, keyset, key, dg, dlen, sg, valid, st))

    def dsa_verify_keyset(self, keyset: int, key: int, digest: bytes, sig: bytes):
        """crypto/dsa.Verify for one raw signature r || s under key `key` of a resident DSA key set -> (rc, status, valid)."""
        if not digest or len(sig) != 2 * self.ctx.dsa_keyset_info(keyset)["qbytes"]:
            raise ValueError("dsa_verify_keyset: sig of 2 qbytes of the set, a non-empty digest")
        return self._verdict(digest, sig, lambda dg, dlen, sg, valid, st: self.lib.bftkv_gpu_batcher_dsa_verify_keyset(
            self.h, keyset, key, dg, dlen, sg, valid, st))

    def rsa_verify(self, digest: bytes, sig: bytes, n: int, e: int, hash_id: int):
        """rsa.VerifyPKCS1v15 for one raw signature (nbytes = len(sig)) under (n, e) -> (rc, status, valid)."""
        if not digest or not sig:
            raise ValueError("rsa_verify: a non-empty digest and signature")
        dg, sg, nn = _u8(digest), _u8(sig), _ints_to_be([n], len(sig))
        valid, st = np.full(1, 0xAA, dtype=np.uint8), np.zeros(1, dtype=np.uint8)
        rc = self.lib.bftkv_gpu_batcher_rsa_verify(self.h, _ptr(dg), hash_id, len(digest), _ptr(sg), len(sig), _ptr(nn), e, _ptr(valid), _ptr(st))
        return rc, int(st[0]), int(valid[0])

    def rsa_verify_keyset(self, keyset: int, key: int, digest: bytes, sig: bytes, hash_id: int):
        """rsa.VerifyPKCS1v15 for one raw signature under key `key` of a resident RSA key set -> (rc, status, valid)."""
        if not digest or len(sig) != self.ctx.rsa_keyset_info(keyset)["nbytes"]:
            raise ValueError("rsa_verify_keyset: sig of the set's nbytes, a non-empty digest")
        return self._verdict(digest, sig, lambda dg, dlen, sg, valid, st: self.lib.bftkv_gpu_batcher_rsa_verify_keyset(
            self.h, keyset, key, dg, hash_id, dlen, sg, valid, st))

    def modexp(self, base: int, exp: int, mod: int, nbytes: int = 256, exp_len: int = 32):
        """base^exp mod `mod` (CalculatePartialR dsa.go:27-31; the per-fragment power of rsa.go:161-171)."""
        b, e, m = _ints_to_be([base], nbytes), _ints_to_be([exp], exp_len), _ints_to_be([mod], nbytes)
        out, st = np.full(nbytes, 0xAA, dtype=np.uint8), np.zeros(1, dtype=np.uint8)
        rc = self.lib.bftkv_gpu_batcher_modexp(self.h, _ptr(b), nbytes, _ptr(e), exp_len, _ptr(m), _ptr(out), _ptr(st))
        return rc, int(st[0]), int.from_bytes(out.tobytes(), "big")

    def tpa_yi(self, x: bytes, y: bytes, mod: bytes):
        """makeYi for one request: x and mod of nbytes, y of exp_len bytes, big-endian -> (rc, status, yi bytes)."""
        xx, yy, m = _u8(x), _u8(y), _u8(mod)
        out, st = np.full(max(1, len(x)), 0xAA, dtype=np.uint8), np.zeros(1, dtype=np.uint8)
        rc = self.lib.bftkv_gpu_batcher_tpa_yi(self.h, _ptr(xx), len(x), _ptr(yy), len(y), _ptr(m), _ptr(out), _ptr(st))
        return rc, int(st[0]), out[:len(x)].tobytes()

    def tpa_bi(self, v: bytes, xi: bytes, b: bytes, salt: bytes, mod: bytes):
        """makeBi for one request: v and mod of nbytes, xi as received (at most nbytes), b of exp_len bytes, salt of at most 64
        -> (rc, status, bi bytes, keys, mac)."""
        vv, bb, m = _u8(v), _u8(b), _u8(mod)
        xx, ss = (_u8(xi) if xi else None), (_u8(salt) if salt else None)
        out, st = np.full(max(1, len(v)), 0xAA, dtype=np.uint8), np.zeros(1, dtype=np.uint8)
        keys, mac = np.full(32, 0xAA, dtype=np.uint8), np.full(32, 0xAA, dtype=np.uint8)
        rc = self.lib.bftkv_gpu_batcher_tpa_bi(self.h, _ptr(vv), _ptr(xx), len(xi), len(v), _ptr(bb), len(b), _ptr(ss), len(salt), _ptr(m), _ptr(out),
                                               _ptr(keys), _ptr(mac), _ptr(st))
        return rc, int(st[0]), out[:len(v)].tobytes(), keys.tobytes(), mac.tobytes()

    def rsa_partial_sign(self, t: bytes, mod: bytes, exps, sign, exp_used=None):
        """rsaContext.Sign for one request with all its fragments: T as received, mod of nbytes, exps [n_frags, exp_len] right-aligned,
        sign [n_frags], exp_used [n_frags] or None -> (rc, status [n_frags], out [n_frags, nbytes])."""
        tt, m, ee, sg = (_u8(t) if t else None), _u8(mod), _u8(exps), _u8(sign)
        n_frags, nbytes = len(sg), len(mod)
        ee = ee.reshape(max(n_frags, 1), -1)
        eu = None if exp_used is None else np.ascontiguousarray(exp_used, dtype=np.uint32)
        out, st = np.full((max(1, n_frags), max(1, nbytes)), 0xAA, dtype=np.uint8), np.zeros(max(1, n_frags), dtype=np.uint8)
        rc = self.lib.bftkv_gpu_batcher_rsa_partial_sign(self.h, _ptr(tt), len(t), _ptr(m), nbytes, n_frags, _ptr(ee), ee.shape[1],
                                                         None if eu is None else eu.ctypes.data, _ptr(sg), _ptr(out), _ptr(st))
        return rc, st[:n_frags].copy(), out.reshape(-1)[:n_frags * nbytes].reshape(n_frags, nbytes).copy()

    def tdsa_share(self, keyset: int, group: int, shares):
        """dsaContext.Sign, phase 2, for one request under group `group` of a resident DSA key set: shares [m, 4, qbytes]
        -> (rc, status, ri, vi, ki, ci) as bytes."""
        info = self.ctx.dsa_keyset_info(keyset)
        pb, qb = info["pbytes"], info["qbytes"]
        sh = np.ascontiguousarray(shares, dtype=np.uint8)
        m, sh = sh.shape[0], _u8(sh.reshape(-1, 4, qb))
        ri, st = np.full(pb, 0xAA, dtype=np.uint8), np.zeros(1, dtype=np.uint8)
        vi, ki, ci = (np.full(qb, 0xAA, dtype=np.uint8) for _ in range(3))
        rc = self.lib.bftkv_gpu_batcher_tdsa_share(self.h, keyset, group, m, _ptr(sh), pb, qb, _ptr(ri), _ptr(vi), _ptr(ki), _ptr(ci), _ptr(st))
        return rc, int(st[0]), ri.tobytes(), vi.tobytes(), ki.tobytes(), ci.tobytes()

    def tecdsa_share(self, shares, curve):
        """dsaContext.Sign, phase 2, for one request on a recognised curve: shares [m, 4, fbytes] -> (rc, status, ri, vi, ki, ci) as bytes."""
        cb, bits, f = _curve_bytes(curve)
        sh = np.ascontiguousarray(shares, dtype=np.uint8)
        m, sh = sh.shape[0], _u8(sh.reshape(-1, 4, f))
        ri, st = np.full(1 + 2 * f, 0xAA, dtype=np.uint8), np.zeros(1, dtype=np.uint8)
        vi, ki, ci = (np.full(f, 0xAA, dtype=np.uint8) for _ in range(3))
        rc = self.lib.bftkv_gpu_batcher_tecdsa_share(self.h, m, _ptr(sh), _ptr(cb), bits, _ptr(ri), _ptr(vi), _ptr(ki), _ptr(ci), _ptr(st))
        return rc, int(st[0]), ri.tobytes(), vi.tobytes(), ki.tobytes(), ci.tobytes()

    def rsa_sign_keyset(self, signer: int, key: int, digest: bytes, hash_id: int):
        """rsa.SignPKCS1v15 for one digest under key `key` of a resident signer set -> (rc, status, signature bytes of the set's nbytes)."""
        nbytes = self.ctx.rsa_signer_info(signer)["nbytes"]
        dg = np.frombuffer(bytes(digest), dtype=np.uint8).copy() if digest else np.zeros(1, dtype=np.uint8)
        sig, st = np.full(nbytes, 0xAA, dtype=np.uint8), np.zeros(1, dtype=np.uint8)
        rc = self.lib.bftkv_gpu_batcher_rsa_sign_keyset(self.h, signer, key, _ptr(dg), len(digest), hash_id, _ptr(sig), _ptr(st))
        return rc, int(st[0]), sig.tobytes()

    def stats(self):
        st = (C.c_uint64 * 4)()
        self.lib.bftkv_gpu_batcher_stats(self.h, st)
        ns = (C.c_uint64 * 8)()
        self.lib.bftkv_gpu_batcher_times(self.h, ns)
        return {"calls": st[0], "batches": st[1], "max_batch": st[2], "lanes": st[3], "cert_fast": ns[7]}


def _curve_bytes(curve):
    """{p, n, b, gx, gy, bit_size} -> (P || N || B || Gx || Gy as uint8, bit_size, fbytes)."""
    bits = int(curve["bit_size"])
    f = (bits + 7) // 8
    return _ints_to_be([int(curve[key]) for key in ("p", "n", "b", "gx", "gy")], f).reshape(-1).copy(), bits, f


def _ints_to_be(vals, nbytes: int) -> np.ndarray:
    return np.frombuffer(b"".join(int(v).to_bytes(nbytes, "big") for v in vals), dtype=np.uint8).reshape(len(vals), nbytes).copy()


def _u8(a) -> np.ndarray:
    if isinstance(a, (bytes, bytearray)):
        a = np.frombuffer(bytes(a), dtype=np.uint8)
    a = np.ascontiguousarray(a, dtype=np.uint8)
    if a.size == 0:
        a = np.zeros(1, dtype=np.uint8)[:0].copy()
    return a


def _u64(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.uint64)
