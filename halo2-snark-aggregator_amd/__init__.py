"""halo2-snark-aggregator_amd — MI355X (gfx950) backend for the pure-calculation hot path of
scroll-tech/halo2-snark-aggregator (BN254 G1 multi_exp + multi-open evaluation).

This module is a thin ctypes binding of the C ABI in include/h2agg.h (libh2agg.so, built from
csrc/*.hip by build_ext.py).  All arithmetic happens in HIP kernels; there is NO CPU fallback:
`load_library()` raises if the shared object is missing and `H2Agg()` raises if no HIP device is
usable.  The directory name contains a hyphen (it mirrors the reference's crate naming), so import it
with `importlib` — see tests/conftest.py / __graft_entry__.py (`load_package()`).
"""
from __future__ import annotations

import ctypes as C
import os
from typing import List, Optional, Sequence

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libh2agg.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "h2agg.h")

OK, ERR_INVALID, ERR_DIV_ZERO, ERR_EMPTY, ERR_HIP, ERR_NONCANONICAL, ERR_NOMEM, ERR_BAD_POINT, ERR_PEER, ERR_NOT_IN_TABLE = range(10)
OP_ADD, OP_SUB, OP_MUL, OP_SQR, OP_INV, OP_DIV = range(6)
FR_FFT_LOCAL = 10    # radix-2 stages h2agg_fr_fft fuses per pass by default (csrc/fr_fft_kernels.hpp)
FR_FFT_MAX_K = 24
FR_QUOTIENT_MAX_K = 28  # h2agg_quotient_device: k + e, the extended domain (the two-adicity of Fr); above 2^24 the coset-split ending
# The grid-stride launches whose workgroup cap goes by the CU count, as (workgroups per CU, elements per workgroup): a lane's
# loop runs a second time above cus * per_cu * per_workgroup elements (cus: the device's count, or the debug key launch_cus)
LAUNCH_ELEMENTWISE = (8, 256)   # grid_for (csrc/host.inc): the element-wise kernels, BLOCK elements per workgroup
LAUNCH_SCALAR_MUL = (16, 32)    # h2agg_g1_batch_scalar_mul (csrc/chips_api.inc) and the comb's table (csrc/bases_api.inc): SM_GROUPS
LAUNCH_SIZE_ORDER = (4, 256)    # k_size_count / k_size_scatter over the buckets of an MSM (csrc/msm_run.inc msm_order)
LAUNCH_MSM_FIX = (12, 64)       # k_msm_accumulate_fix over the lean accumulation's fix-up list (csrc/msm_run.inc msm_big_kernels)
LAUNCH_MSM_BIG = (8, 64)        # k_msm_accumulate_big / k_msm_big_combine: one-wave workgroups, one list entry per workgroup
FR_POLY_CHUNK = 11   # log2 of the coefficients per workgroup of the KZG opening kernels by default (csrc/fr_chunk.hpp)
FR_SCAN_CHUNK = 11   # log2 of the elements per workgroup of the grand-product kernels by default (csrc/fr_chunk.hpp)
FR_PROD_MAX_COLUMNS = 16
FR_SORT_TILE = 11    # log2 of the keys per workgroup of the lookup permutation by default (csrc/lookup_kernels.hpp)
FR_SORT_TILE_MIN = 4
LOOKUP_STATUS_NONCANONICAL, LOOKUP_STATUS_NOT_IN_TABLE = 1, 8   # the bits of a lookup batch's status words (include/h2agg.h)
FR_COMPRESS_MAX_COLUMNS = 1 << 16   # most columns of one fr_columns_compress (the library's limit: csrc/lookup.inc)
PERM_MAX_COLUMNS = 4096   # H2AGG_PERM_MAX_COLUMNS: most columns of one permutation (csrc/keygen_kernels.hpp)
EXPR_MAX_DEPTH = 16  # H2AGG_EXPR_MAX_DEPTH: the operand stack of h2agg_vk_expressions_eval / h2agg_quotient (csrc/quotient_kernels.hpp)
WC_GATES, WC_PERMUTATION, WC_LOOKUPS = 1, 2, 4   # H2AGG_WC_*: the kinds of constraint h2agg_witness_check checks
WC_NONE = 0xFFFFFFFF   # "no row" in its report
PK_COSETS = 1   # H2AGG_PK_COSETS: the proving key also holds its columns' values on every coset of the extended domain
# H2AGG_PK_*: the forms h2agg_pk_ptr answers
PK_FIXED_LAGRANGE, PK_SIGMA_LAGRANGE, PK_FIXED_COEFF, PK_SIGMA_COEFF, PK_LAGRANGE_COEFF, PK_COSET = range(6)

IDENTITY_JAC =(0).to_bytes(32, "little") + (1).to_bytes(32, "little") + (0).to_bytes(32, "little")


class H2AggError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__("h2agg error %d: %s" % (code, msg))
        self.code = code


class EmptyMultiExp(H2AggError):
    """multi_exp of zero pairs — the reference panics (`acc.unwrap()`, mock/arith/ecc.rs:128)."""


class BadPoint(H2AggError, ValueError):
    """"invalid point encoding in proof" (systems/halo2/transcript.rs:65-70)."""


class DivisionByZero(H2AggError, ZeroDivisionError):
    """inversion of zero — the reference panics (`invert().unwrap()`, mock/arith/field.rs:113)."""


_lib = None


def load_library():
    """dlopen libh2agg.so and declare every prototype.  Fails loudly if the extension is not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            "libh2agg.so is not built (%s). Run `python __graft_entry__.py build` — the HIP extension is "
            "required, there is no CPU fallback." % LIB_PATH)
    # PyTorch-ROCm ships its own copy of the HIP runtime.  Whichever copy is loaded first serves the whole process: with
    # libh2agg.so first (the system's /opt/rocm runtime), a later `import torch` finds "No HIP GPUs are available".  The
    # harness uses torch for device memory and streams anyway, so let it load its runtime before the library binds to it.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = C.CDLL(LIB_PATH)
    u8p, vp, sz, i32, u64 = C.c_char_p, C.c_void_p, C.c_size_t, C.c_int, C.c_uint64
    ctxp = C.c_void_p
    protos = {
        "h2agg_create": (i32, [i32, C.POINTER(ctxp)]),
        "h2agg_destroy": (None, [ctxp]),
        "h2agg_last_error": (C.c_char_p, [ctxp]),
        "h2agg_set_stream": (i32, [ctxp, vp]),
        "h2agg_synchronize": (i32, [ctxp]),
        "h2agg_describe": (C.c_char_p, [ctxp]),
        "h2agg_fr_batch_op": (i32, [ctxp, i32, u8p, u8p, sz, vp]),
        "h2agg_fr_batch_pow_constant": (i32, [ctxp, u8p, sz, u64, vp]),
        "h2agg_fr_tape_eval": (i32, [ctxp, u8p, sz, vp, sz, vp, sz, vp]),
        "h2agg_fr_mul_add_accumulate": (i32, [ctxp, u8p, sz, u8p, vp]),
        "h2agg_fr_sum_with_coeff_and_constant": (i32, [ctxp, u8p, u8p, sz, u8p, vp]),
        "h2agg_g1_batch_add": (i32, [ctxp, u8p, u8p, sz, i32, vp]),
        "h2agg_g1_batch_scalar_mul": (i32, [ctxp, u8p, u8p, sz, vp]),
        "h2agg_g1_batch_to_affine": (i32, [ctxp, u8p, sz, vp]),
        "h2agg_g1_sum": (i32, [ctxp, u8p, sz, vp]),
        "h2agg_g1_batch_decompress": (i32, [ctxp, u8p, sz, vp, vp]),
        "h2agg_g1_batch_compress": (i32, [ctxp, u8p, sz, vp]),
        "h2agg_g1_msm": (i32, [ctxp, vp, vp, sz, vp]),
        "h2agg_g1_msm_jac": (i32, [ctxp, vp, vp, sz, vp]),
        "h2agg_g1_msm_segmented": (i32, [ctxp, vp, vp, sz, C.POINTER(u64), sz, vp]),
        "h2agg_host_alloc": (i32, [ctxp, sz, C.POINTER(vp)]),
        "h2agg_host_free": (i32, [ctxp, vp]),
        "h2agg_eval_flat": (i32, [ctxp, u8p, u8p, u8p, sz, vp]),
        "h2agg_bases_upload": (i32, [ctxp, u8p, sz, C.POINTER(u64)]),
        "h2agg_bases_generate": (i32, [ctxp, vp, sz, C.POINTER(u64)]),
        "h2agg_bases_precompute": (i32, [ctxp, u64, i32]),
        "h2agg_bases_download": (i32, [ctxp, u64, sz, sz, vp]),
        "h2agg_bases_free": (i32, [ctxp, u64]),
        "h2agg_g1_msm_preloaded": (i32, [ctxp, u64, u8p, sz, vp]),
        "h2agg_instance_commitment": (i32, [ctxp, u64, u8p, sz, sz, vp]),
        "h2agg_g1_msm_device": (i32, [ctxp, u64, vp, sz, vp]),
        "h2agg_g1_msm_device_async": (i32, [ctxp, u64, vp, sz, vp]),
        "h2agg_schema_create": (i32, [ctxp, C.POINTER(C.c_void_p)]),
        "h2agg_schema_destroy": (None, [C.c_void_p]),
        "h2agg_schema_node_commitment": (i32, [C.c_void_p, C.c_char_p, u8p, C.POINTER(C.c_uint32)]),
        "h2agg_schema_node_eval": (i32, [C.c_void_p, u8p, C.POINTER(C.c_uint32)]),
        "h2agg_schema_node_scalar": (i32, [C.c_void_p, u8p, C.POINTER(C.c_uint32)]),
        "h2agg_schema_node_add": (i32, [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32)]),
        "h2agg_schema_node_mul": (i32, [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32)]),
        "h2agg_schema_estimate": (i32, [C.c_void_p, C.c_uint32, C.POINTER(C.c_size_t)]),
        "h2agg_schema_evaluation_queries": (i32, [C.c_void_p, sz, C.POINTER(C.c_char_p), u8p, u8p,
                                                  C.POINTER(C.c_uint32)]),
        "h2agg_schema_batch_multi_open": (i32, [C.c_void_p, C.c_char_p, sz, C.POINTER(C.c_int32), u8p,
                                                C.POINTER(C.c_uint32), sz, u8p, u8p, u8p,
                                                C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
        "h2agg_schema_shplonk_multi_open": (i32, [C.c_void_p, C.c_char_p, sz, C.POINTER(C.c_uint32), C.POINTER(C.c_int32), u8p,
                                                  C.POINTER(C.c_uint32), u8p, u8p, u8p, u8p, u8p,
                                                  C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
        "h2agg_schema_eval": (i32, [C.c_void_p, C.c_uint32, vp, C.POINTER(i32), vp]),
        "h2agg_evaluate_multiopen_proof": (i32, [C.c_void_p, C.c_uint32, C.c_uint32, vp, vp]),
        "h2agg_evaluate_multiopen_prepare": (i32, [C.c_void_p, C.c_uint32, C.c_uint32]),
        "h2agg_schema_name_count": (C.c_size_t, [C.c_void_p]),
        "h2agg_schema_name": (C.c_char_p, [C.c_void_p, C.c_size_t]),
        "h2agg_g1_msm_device_batch_async": (C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p]),
        "h2agg_schema_query_set_commitment": (C.c_int, [C.c_void_p, C.c_uint32, C.c_char_p]),
        "h2agg_g1_batch_to_affine_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_char_p]),
        "h2agg_schema_names_joined": (C.c_size_t, [C.c_void_p, C.c_char_p, C.c_size_t]),
        "h2agg_schema_point_list_len": (C.c_size_t, [C.c_void_p]),
        "h2agg_poseidon_squeeze_batch": (i32, [ctxp, u8p, sz, sz, C.POINTER(C.c_uint32), sz, vp]),
        "h2agg_transcript_read_batch": (i32, [ctxp, u8p, sz, sz, C.c_char_p, sz, u8p, sz, u8p, sz, vp, vp]),
        "h2agg_vk_create": (i32, [ctxp, u8p, sz, C.POINTER(C.c_void_p)]),
        "h2agg_vk_set_transcript": (i32, [C.c_void_p, i32]),
        "h2agg_vk_set_multiopen": (i32, [C.c_void_p, i32]),
        "h2agg_hash_transcript_read_batch": (i32, [ctxp, i32, u8p, sz, sz, C.c_char_p, sz, u8p, sz, u8p, sz, vp, vp]),
        "h2agg_hash_transcript_read_batch_host": (i32, [i32, u8p, sz, sz, C.c_char_p, sz, u8p, sz, u8p, sz, vp, vp, i32]),
        "h2agg_hash_digest_host": (i32, [i32, u8p, sz, vp]),
        "h2agg_vk_destroy": (None, [C.c_void_p]),
        "h2agg_verify_aggregation": (i32, [ctxp, vp, sz, u8p, u8p, vp, vp, vp, C.POINTER(i32)]),   # see verifier.py
        "h2agg_verify_aggregation_ex": (i32, [ctxp, vp, sz, u8p, u8p, vp, vp, vp, C.POINTER(i32), vp, sz]),
        "h2agg_verify_aggregation_sharded": (i32, [ctxp, vp, sz, vp, u8p, u8p, vp, vp, vp, C.POINTER(i32), vp, sz]),   # see verifier.py
        "h2agg_debug_configure": (i32, [ctxp, C.c_char_p, i32]),
        "h2agg_debug_lean_variant": (i32, [i32, i32]),
        "h2agg_debug_table_identity": (i32, [ctxp, u64, C.POINTER(i32), C.POINTER(i32)]),
        "h2agg_verify_proofs": (i32, [ctxp, vp, sz, u8p, u8p, vp, vp, C.POINTER(C.c_int32), C.POINTER(i32), vp, sz]),
        "h2agg_verify_plan_stats": (i32, [ctxp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
        "h2agg_last_phases": (C.c_char_p, [ctxp]),
        "h2agg_transcript_configure": (i32, [ctxp, i32]),
        "h2agg_poseidon_squeeze_batch_host": (i32, [u8p, sz, sz, C.POINTER(C.c_uint32), sz, vp, i32]),
        "h2agg_host_threads": (i32, []),
        "h2agg_host_sponge_kind": (i32, []),
        "h2agg_comm_unique_id": (i32, [vp]),
        "h2agg_comm_init_rank": (i32, [ctxp, u8p, i32, i32]),
        "h2agg_comm_create": (i32, [C.POINTER(i32), i32, C.POINTER(ctxp)]),
        "h2agg_comm_size": (i32, [ctxp]),
        "h2agg_comm_rank": (i32, [ctxp]),
        "h2agg_comm_last_error": (C.c_char_p, []),
        "h2agg_allgather_add_points": (i32, [C.POINTER(ctxp), i32, u8p, sz, vp]),
        "h2agg_pairing_check": (i32, [ctxp, u8p, u8p, sz, C.POINTER(i32)]),
        "h2agg_g2_batch_decompress": (i32, [ctxp, u8p, sz, vp]),
        "h2agg_bases_fft": (i32, [ctxp, u64, C.c_uint, i32, C.POINTER(u64)]),
        "h2agg_params_setup": (i32, [ctxp, C.c_uint, u8p, C.POINTER(u64), C.POINTER(u64)]),
        "h2agg_fr_fft": (i32, [ctxp, vp, C.c_uint, i32, u8p, vp]),
        "h2agg_fr_fft_device": (i32, [ctxp, vp, C.c_uint, i32, u8p, vp]),
        "h2agg_fr_fft_batch": (i32, [ctxp, vp, C.c_size_t, C.c_uint, i32, u8p, vp]),
        "h2agg_fr_poly_eval": (i32, [ctxp, vp, sz, C.c_uint, C.POINTER(C.c_uint32), sz, u8p, sz, vp]),
        "h2agg_fr_poly_eval_device": (i32, [ctxp, vp, sz, C.c_uint, C.POINTER(C.c_uint32), sz, u8p, sz, vp]),
        "h2agg_fr_poly_divide": (i32, [ctxp, vp, C.c_uint, u8p, vp, vp]),
        "h2agg_fr_poly_divide_device": (i32, [ctxp, vp, C.c_uint, u8p, vp, vp]),
        "h2agg_kzg_multiopen": (i32, [ctxp, u64, vp, sz, C.c_uint, C.POINTER(C.c_uint32), sz, u8p, sz, u8p, vp,
                                      C.POINTER(C.c_uint32), C.POINTER(sz)]),
        "h2agg_kzg_multiopen_device": (i32, [ctxp, u64, vp, sz, C.c_uint, C.POINTER(C.c_uint32), sz, u8p, sz, u8p, vp,
                                             C.POINTER(C.c_uint32), C.POINTER(sz)]),
        "h2agg_kzg_shplonk_begin": (i32, [ctxp, u64, vp, sz, C.c_uint, C.POINTER(C.c_uint32), sz, u8p, sz, u8p, u8p, u8p, vp,
                                          C.POINTER(vp)]),
        "h2agg_kzg_shplonk_finish": (i32, [vp, u8p, vp]),
        "h2agg_kzg_shplonk_destroy": (None, [vp]),
        "h2agg_fr_batch_invert": (i32, [ctxp, vp, sz, vp]),
        "h2agg_fr_batch_invert_device": (i32, [ctxp, vp, sz, vp]),
        "h2agg_fr_grand_product": (i32, [ctxp, vp, vp, C.c_uint, sz, u8p, vp, vp]),
        "h2agg_fr_grand_product_device": (i32, [ctxp, vp, vp, C.c_uint, sz, u8p, vp, vp]),
        "h2agg_permutation_product": (i32, [ctxp, vp, vp, sz, C.c_uint, sz, u8p, u8p, u8p, u8p, u8p, vp, vp]),
        "h2agg_permutation_product_device": (i32, [ctxp, vp, vp, sz, C.c_uint, sz, u8p, u8p, u8p, u8p, u8p, vp, vp]),
        "h2agg_lookup_product": (i32, [ctxp, vp, vp, vp, vp, C.c_uint, sz, u8p, u8p, vp, vp]),
        "h2agg_lookup_product_device": (i32, [ctxp, vp, vp, vp, vp, C.c_uint, sz, u8p, u8p, vp, vp]),
        "h2agg_lookup_permute": (i32, [ctxp, vp, vp, C.c_uint, sz, vp, vp]),
        "h2agg_lookup_permute_device": (i32, [ctxp, vp, vp, C.c_uint, sz, vp, vp]),
        "h2agg_lookup_batch_permute": (i32, [ctxp, vp, vp, sz, C.c_uint, sz, vp, vp, vp]),
        "h2agg_lookup_batch_product": (i32, [ctxp, vp, vp, vp, vp, sz, C.c_uint, sz, u8p, u8p, vp, vp]),
        "h2agg_lookup_store_permute": (i32, [ctxp, u64, sz, u64, sz, sz, sz, u64, sz, u64, sz, vp]),
        "h2agg_lookup_store_product": (i32, [ctxp, u64, sz, u64, sz, u64, sz, u64, sz, sz, sz, u8p, u8p, u64, sz, vp]),
        "h2agg_lookup_configure": (i32, [ctxp, sz]),
        "h2agg_lookup_chunk_rule": (sz, [sz, sz]),
        "h2agg_fr_columns_compress": (i32, [ctxp, vp, sz, C.c_uint, u8p, vp]),
        "h2agg_fr_columns_compress_device": (i32, [ctxp, vp, sz, C.c_uint, u8p, vp]),
        "h2agg_vk_expressions_eval": (i32, [ctxp, vp, i32, sz, C.c_uint, vp, vp, vp, u8p, u8p, vp]),
        "h2agg_vk_expressions_eval_device": (i32, [ctxp, vp, i32, sz, C.c_uint, vp, vp, vp, u8p, u8p, vp]),
        "h2agg_quotient": (i32, [ctxp, vp, vp, vp, vp, vp, vp, vp, vp, vp, u8p, u8p, u8p, u8p, u8p, u8p, vp]),
        "h2agg_quotient_device": (i32, [ctxp, vp, vp, vp, vp, vp, vp, vp, vp, vp, u8p, u8p, u8p, u8p, u8p, u8p, vp]),
        "h2agg_quotient_configure": (i32, [ctxp, i32]),
        "h2agg_quotient_work_bytes": (i32, [vp, C.POINTER(sz)]),
        "h2agg_permutation_assembly": (i32, [sz, C.c_uint, sz, vp, sz, vp]),
        "h2agg_permutation_sigmas": (i32, [ctxp, vp, sz, C.c_uint, sz, u8p, vp, vp]),
        "h2agg_commit_columns": (i32, [ctxp, u64, vp, sz, C.c_uint, vp]),
        "h2agg_witness_check_layout": (i32, [vp, C.POINTER(sz), C.POINTER(sz), C.POINTER(sz)]),
        "h2agg_witness_check": (i32, [ctxp, vp, C.c_uint, vp, vp, vp, u8p, u8p, vp, sz, vp, vp, vp, C.POINTER(u64)]),
        "h2agg_columns_create": (i32, [ctxp, sz, C.c_uint, C.POINTER(u64)]),
        "h2agg_columns_destroy": (i32, [ctxp, u64]),
        "h2agg_columns_info": (i32, [ctxp, u64, C.POINTER(sz), C.POINTER(C.c_uint)]),
        "h2agg_columns_write": (i32, [ctxp, u64, sz, sz, vp]),
        "h2agg_columns_read": (i32, [ctxp, u64, sz, sz, vp]),
        "h2agg_columns_ptr": (i32, [ctxp, u64, sz, C.POINTER(vp)]),
        "h2agg_columns_move": (i32, [ctxp, u64, sz, u64, sz, sz, C.c_int32]),
        "h2agg_columns_fft": (i32, [ctxp, u64, sz, u64, sz, sz, i32, u8p]),
        "h2agg_columns_commit": (i32, [ctxp, u64, u64, sz, sz, vp]),
        "h2agg_columns_sigmas": (i32, [ctxp, vp, sz, C.c_uint, sz, u8p, u64, sz, u64, sz]),
        "h2agg_columns_witness_check": (i32, [ctxp, vp, C.c_uint, u64, sz, u64, sz, u64, sz, u8p, u8p, vp, sz, vp, vp, vp,
                                              C.POINTER(u64)]),
        "h2agg_columns_shplonk_begin": (i32, [ctxp, u64, u64, sz, sz, C.POINTER(C.c_uint32), sz, u8p, sz, u8p, u8p, u8p, vp,
                                              C.POINTER(vp)]),
        "h2agg_pk_create": (i32, [ctxp, vp, vp, vp, C.c_uint, C.POINTER(vp)]),
        "h2agg_pk_create_resident": (i32, [ctxp, vp, vp, vp, C.c_uint, C.POINTER(vp)]),
        "h2agg_pk_bytes": (i32, [vp, C.c_uint, C.POINTER(sz)]),
        "h2agg_pk_info": (i32, [vp, C.POINTER(C.c_uint), C.POINTER(C.c_uint), C.POINTER(sz), C.POINTER(sz), C.POINTER(C.c_uint),
                                C.POINTER(sz)]),
        "h2agg_pk_ptr": (i32, [vp, i32, sz, C.POINTER(vp), C.POINTER(sz)]),
        "h2agg_pk_quotient": (i32, [ctxp, vp, vp, vp, vp, vp, vp, vp, u8p, u8p, u8p, u8p, u8p, u8p, vp]),
        "h2agg_pk_quotient_work_bytes": (i32, [vp, C.POINTER(sz)]),
        "h2agg_pk_destroy": (None, [vp]),
        "h2agg_g2_scalar_mul": (i32, [u8p, u8p, vp]),
        "h2agg_g2_batch_compress": (i32, [u8p, sz, vp]),
        "h2agg_pairing_product": (i32, [ctxp, u8p, u8p, sz, vp]),
        "h2agg_final_pair_check": (i32, [ctxp, u8p, u8p, u8p, u8p, C.POINTER(i32)]),
        "h2agg_msm_configure": (i32, [ctxp, i32, i32, i32]),
        "h2agg_msm_configure_glv": (i32, [ctxp, i32]),
        "h2agg_msm_configure_lanes_per_bucket": (i32, [ctxp, i32]),
        "h2agg_msm_configure_sort": (i32, [ctxp, i32, i32]),
        "h2agg_msm_set_tail_overlap": (i32, [ctxp, i32]),
        "h2agg_profile_enable": (i32, [ctxp, i32]),
        "h2agg_profile_reset": (i32, [ctxp]),
        "h2agg_profile_stage_count": (i32, [ctxp]),
        "h2agg_profile_stage_name": (C.c_char_p, [ctxp, i32]),
        "h2agg_profile_stage_get": (i32, [ctxp, i32, C.POINTER(C.c_double), C.POINTER(u64)]),
    }
    for name, (res, args) in protos.items():
        fn = getattr(lib, name)  # AttributeError if the library does not export a declared symbol
        fn.restype = res
        fn.argtypes = args
    lib._h2agg_protos = tuple(protos)
    _lib = lib
    return lib


def exported_symbols() -> Sequence[str]:
    return load_library()._h2agg_protos


def _need(buf, nbytes: int, what: str):
    """the C side trusts the lengths it is given: a short Python buffer would be read past its end"""
    if buf is None or len(buf) != nbytes:
        raise ValueError("%s must be exactly %d bytes (got %s)" % (what, nbytes, "None" if buf is None else len(buf)))


def _check_host(rc: int, what: str):
    if rc == ERR_BAD_POINT:
        raise BadPoint(rc, what + ": invalid G2 point")
    if rc != OK:
        raise H2AggError(rc, what + (": input integer >= modulus" if rc == ERR_NONCANONICAL else " failed"))


def g2_scalar_mul(g2_aff: bytes, s: bytes) -> bytes:
    """h2agg_g2_scalar_mul: host arithmetic, no context"""
    _need(g2_aff, 128, "g2_aff")
    _need(s, 32, "s")
    out = C.create_string_buffer(128)
    _check_host(load_library().h2agg_g2_scalar_mul(g2_aff, s, out), "g2_scalar_mul")
    return out.raw


def _words(data, nwords: int, what: str):
    """uint32 words for the C side: bytes / bytearray (little-endian words), an array('I'), a ctypes array of c_uint32, or
    a sequence of integers -> a ctypes array of exactly nwords words"""
    if isinstance(data, (bytes, bytearray, memoryview)):
        _need(data, 4 * nwords, what)
        return (C.c_uint32 * max(nwords, 1)).from_buffer_copy(bytes(data) if nwords else bytes(4))
    if isinstance(data, C.Array) and data._type_ is C.c_uint32:
        if len(data) != nwords:
            raise ValueError("%s must be exactly %d words (got %d)" % (what, nwords, len(data)))
        return data
    if data is None or len(data) != nwords:
        raise ValueError("%s must be exactly %d words (got %s)" % (what, nwords, "None" if data is None else len(data)))
    return (C.c_uint32 * max(nwords, 1))(*data)


def _perm_shape_ok(m: int, k: int, usable: int) -> bool:
    """the shapes the library goes on to read buffers for (it refuses the others before it touches one)"""
    return 0 <= k <= FR_FFT_MAX_K and 1 <= m <= PERM_MAX_COLUMNS and 0 <= usable <= (1 << k)


def permutation_assembly(m: int, k: int, usable: int, copies) -> bytes:
    """h2agg_permutation_assembly: host arithmetic, no context.  copies: quadruples (left column, left row, right column,
    right row), as a sequence of 4-tuples or flat words (bytes, array('I'), ctypes).  -> the mapping halo2's Assembly holds
    after copy() on them in order: 2 * m * 2^k little-endian uint32 words, cell (j, i) at pair j * 2^k + i."""
    flat = isinstance(copies, (bytes, bytearray, memoryview, C.Array))
    if not flat:
        copies = list(copies or ())
        if copies and hasattr(copies[0], "__len__"):
            if any(len(q) != 4 for q in copies):
                raise ValueError("a copy is (left column, left row, right column, right row)")
            copies = [int(x) for q in copies for x in q]
    per_copy = 16 if isinstance(copies, (bytes, bytearray, memoryview)) else 4
    if len(copies) % per_copy:
        raise ValueError("copies must be whole quadruples of uint32 words")
    nwords = len(copies) // per_copy * 4
    arr = _words(copies, nwords, "copies")
    out = (C.c_uint32 * (2 * m << k))() if _perm_shape_ok(m, k, usable) else (C.c_uint32 * 1)()
    _check_host(load_library().h2agg_permutation_assembly(m, k, usable, arr, nwords // 4, out), "permutation_assembly")
    return bytes(out)


def g2_batch_compress(aff: bytes) -> bytes:
    """h2agg_g2_batch_compress: host arithmetic, no context"""
    n = len(aff) // 128
    _need(aff, 128 * n, "aff")
    out = C.create_string_buffer(max(64 * n, 1))
    _check_host(load_library().h2agg_g2_batch_compress(aff, n, out), "g2_batch_compress")
    return out.raw[:64 * n]


class H2Agg:
    """One context = one GPU, single-thread-affine (mirrors `MockEccChip::default()` +
    `MockFieldChip::default()` + `MockChipCtx::default()`, verify_circuit.rs:115-118)."""

    def __init__(self, device: int = 0):
        self._lib = load_library()
        self._ctx = C.c_void_p()
        rc = self._lib.h2agg_create(int(device), C.byref(self._ctx))
        if rc != OK:
            self._ctx = None
            raise H2AggError(rc, "h2agg_create(device=%d) failed: a HIP device is required (no CPU mode)" % device)
        self.device = device

    # ------------------------------------------------------------------ plumbing
    def close(self):
        if getattr(self, "_ctx", None):
            for ref in list(getattr(self, "_builders", ())):   # schemas hold device buffers of this context
                b = ref()
                if b is not None:
                    b.close()
            self._lib.h2agg_destroy(self._ctx)
            self._ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _register_builder(self, b):
        import weakref
        if not hasattr(self, "_builders"):
            self._builders = []
        self._builders = [r for r in self._builders if r() is not None]
        self._builders.append(weakref.ref(b))

    def _check(self, rc: int):
        if rc == OK:
            return
        msg = (self._lib.h2agg_last_error(self._ctx) or b"").decode()
        if rc == ERR_EMPTY:
            raise EmptyMultiExp(rc, msg)
        if rc == ERR_DIV_ZERO:
            raise DivisionByZero(rc, msg)
        if rc == ERR_BAD_POINT:
            raise BadPoint(rc, msg)
        raise H2AggError(rc, msg)

    def describe(self) -> str:
        return self._lib.h2agg_describe(self._ctx).decode()

    def set_stream(self, stream_ptr: Optional[int]):
        """a hipStream_t handle for every launch of this context; None or 0 = the context's OWN non-blocking stream.  torch's
        default stream has the handle 0: `set_stream(torch.cuda.current_stream().cuda_stream)` therefore does NOT put the
        library on torch's stream — make a real one (`torch.cuda.Stream()`, `torch.cuda.set_stream`) or synchronise before
        handing device buffers over (include/h2agg.h)."""
        self._check(self._lib.h2agg_set_stream(self._ctx, stream_ptr))

    def synchronize(self):
        self._check(self._lib.h2agg_synchronize(self._ctx))

    # ------------------------------------------------------------------ Fr
    def fr_batch_op(self, op: int, a: bytes, b: Optional[bytes] = None) -> bytes:
        n = len(a) // 32
        _need(a, 32 * n, "a")
        if op in (OP_ADD, OP_SUB, OP_MUL, OP_DIV):
            _need(b, 32 * n, "b")
        out = C.create_string_buffer(32 * n) if n else C.create_string_buffer(1)
        self._check(self._lib.h2agg_fr_batch_op(self._ctx, op, a, b, n, out))
        return out.raw[:32 * n]

    def fr_batch_pow_constant(self, a: bytes, exponent: int) -> bytes:
        n = len(a) // 32
        _need(a, 32 * n, "a")
        out = C.create_string_buffer(max(32 * n, 1))
        self._check(self._lib.h2agg_fr_batch_pow_constant(self._ctx, a, n, exponent, out))
        return out.raw[:32 * n]

    def fr_tape_eval(self, consts: bytes, ops: Sequence, out_regs: Sequence[int]) -> bytes:
        """ops: (opcode, a, b) triples (0 = mul, 1 = add, 2 = sub); registers: inputs first, then one per op"""
        nconst, nops, nout = len(consts) // 32, len(ops), len(out_regs)
        _need(consts, 32 * nconst, "consts")
        flat = (C.c_uint32 * max(3 * nops, 1))(*[x for op in ops for x in op])
        regs = (C.c_uint32 * max(nout, 1))(*out_regs)
        out = C.create_string_buffer(max(32 * nout, 1))
        self._check(self._lib.h2agg_fr_tape_eval(self._ctx, consts, nconst, flat, nops, regs, nout, out))
        return out.raw[:32 * nout]

    def fr_mul_add_accumulate(self, v: bytes, b: bytes) -> bytes:
        _need(v, 32 * (len(v) // 32), "v")
        _need(b, 32, "b")
        out = C.create_string_buffer(32)
        self._check(self._lib.h2agg_fr_mul_add_accumulate(self._ctx, v, len(v) // 32, b, out))
        return out.raw

    def fr_sum_with_coeff_and_constant(self, x: bytes, coeff: bytes, b: bytes) -> bytes:
        _need(x, 32 * (len(x) // 32), "x")
        _need(coeff, len(x), "coeff")
        _need(b, 32, "b")
        out = C.create_string_buffer(32)
        self._check(self._lib.h2agg_fr_sum_with_coeff_and_constant(self._ctx, x, coeff, len(x) // 32, b, out))
        return out.raw

    # ------------------------------------------------------------------ G1 batch
    def g1_batch_add(self, a_jac: bytes, b_jac: bytes, subtract: bool = False) -> bytes:
        n = len(a_jac) // 96
        _need(a_jac, 96 * n, "a_jac")
        _need(b_jac, 96 * n, "b_jac")
        out = C.create_string_buffer(max(96 * n, 1))
        self._check(self._lib.h2agg_g1_batch_add(self._ctx, a_jac, b_jac, n, int(subtract), out))
        return out.raw[:96 * n]

    def g1_batch_scalar_mul(self, bases_aff: bytes, scalars: bytes) -> bytes:
        n = len(scalars) // 32
        _need(scalars, 32 * n, "scalars")
        _need(bases_aff, 64 * n, "bases_aff")
        out = C.create_string_buffer(max(96 * n, 1))
        self._check(self._lib.h2agg_g1_batch_scalar_mul(self._ctx, bases_aff, scalars, n, out))
        return out.raw[:96 * n]

    def g1_batch_to_affine(self, jac: bytes) -> bytes:
        n = len(jac) // 96
        _need(jac, 96 * n, "jac")
        out = C.create_string_buffer(max(64 * n, 1))
        self._check(self._lib.h2agg_g1_batch_to_affine(self._ctx, jac, n, out))
        return out.raw[:64 * n]

    def g1_batch_to_affine_device(self, d_jac_ptr: int, n: int) -> bytes:
        out = C.create_string_buffer(64 * n)
        self._check(self._lib.h2agg_g1_batch_to_affine_device(self._ctx, C.c_void_p(d_jac_ptr), n, out))
        return out.raw

    def g1_batch_decompress(self, data: bytes, with_ok: bool = False):
        """proof wire format -> canonical affine (transcript.rs:63-70); raises BadPoint unless with_ok"""
        n = len(data) // 32
        _need(data, 32 * n, "data")
        out, ok = C.create_string_buffer(max(64 * n, 1)), C.create_string_buffer(max(n, 1))
        rc = self._lib.h2agg_g1_batch_decompress(self._ctx, data, n, out, ok)
        if with_ok and rc in (OK, ERR_BAD_POINT):
            return out.raw[:64 * n], ok.raw[:n]
        self._check(rc)
        return out.raw[:64 * n]

    def g1_batch_compress(self, aff: bytes) -> bytes:
        n = len(aff) // 64
        _need(aff, 64 * n, "aff")
        out = C.create_string_buffer(max(32 * n, 1))
        self._check(self._lib.h2agg_g1_batch_compress(self._ctx, aff, n, out))
        return out.raw[:32 * n]

    def g1_sum(self, jac: bytes) -> bytes:
        _need(jac, 96 * (len(jac) // 96), "jac")
        out = C.create_string_buffer(96)
        self._check(self._lib.h2agg_g1_sum(self._ctx, jac, len(jac) // 96, out))
        return out.raw

    # ------------------------------------------------------------------ MSM
    def g1_msm(self, bases_aff, scalars, n: Optional[int] = None) -> bytes:
        """bases_aff / scalars: bytes, or addresses of host buffers (e.g. from host_alloc) together with n"""
        out = C.create_string_buffer(96)
        if n is None:
            n = len(scalars) // 32
        if isinstance(scalars, (bytes, bytearray)):
            _need(scalars, 32 * n, "scalars")
        if isinstance(bases_aff, (bytes, bytearray)):
            _need(bases_aff, 64 * n, "bases_aff")
        pb = C.cast(bases_aff, C.c_void_p) if isinstance(bases_aff, (bytes, bytearray)) else C.c_void_p(bases_aff)
        ps = C.cast(scalars, C.c_void_p) if isinstance(scalars, (bytes, bytearray)) else C.c_void_p(scalars)
        self._check(self._lib.h2agg_g1_msm(self._ctx, pb, ps, n, out))
        return out.raw

    def g1_msm_jac(self, points_jac: bytes, scalars: bytes) -> bytes:
        """multi_exp over projective points (x || y || z, 96 B each): normalised on the device"""
        n = len(scalars) // 32
        _need(scalars, 32 * n, "scalars")
        _need(points_jac, 96 * n, "points_jac")
        out = C.create_string_buffer(96)
        self._check(self._lib.h2agg_g1_msm_jac(self._ctx, C.cast(points_jac, C.c_void_p), C.cast(scalars, C.c_void_p), n, out))
        return out.raw

    def g1_msm_segmented(self, bases_aff: bytes, scalars: bytes, seg_lens: Sequence[int]) -> List[bytes]:
        """h2agg_g1_msm_segmented: one multi_exp per segment of seg_lens[s] consecutive (base, scalar) pairs, one set of
        device launches for all of them -> a 96-byte Jacobian result per segment"""
        n = len(scalars) // 32
        _need(scalars, 32 * n, "scalars")
        _need(bases_aff, 64 * n, "bases_aff")
        starts = [0]
        for ln in seg_lens:
            starts.append(starts[-1] + int(ln))
        nseg = len(seg_lens)
        seg = (C.c_uint64 * len(starts))(*starts)
        out = C.create_string_buffer(96 * max(nseg, 1))
        self._check(self._lib.h2agg_g1_msm_segmented(self._ctx, C.cast(bases_aff, C.c_void_p), C.cast(scalars, C.c_void_p), n,
                                                     seg, nseg, out))
        raw = out.raw   # (one copy of the buffer, not one per segment)
        return [raw[96 * s: 96 * (s + 1)] for s in range(nseg)]

    def host_alloc(self, nbytes: int) -> int:
        p = C.c_void_p()
        self._check(self._lib.h2agg_host_alloc(self._ctx, nbytes, C.byref(p)))
        return p.value

    def host_free(self, ptr: int):
        self._check(self._lib.h2agg_host_free(self._ctx, C.c_void_p(ptr)))

    def eval_flat(self, pts_aff: bytes, scalars: bytes, has_scalar: bytes) -> bytes:
        n = len(has_scalar)
        _need(pts_aff, 64 * n, "pts_aff")
        _need(scalars, 32 * n, "scalars")
        out = C.create_string_buffer(96)
        self._check(self._lib.h2agg_eval_flat(self._ctx, pts_aff, scalars, has_scalar, len(has_scalar), out))
        return out.raw

    def bases_upload(self, bases_aff: bytes) -> int:
        _need(bases_aff, 64 * (len(bases_aff) // 64), "bases_aff")
        h = C.c_uint64()
        self._check(self._lib.h2agg_bases_upload(self._ctx, bases_aff, len(bases_aff) // 64, C.byref(h)))
        return h.value

    def bases_generate(self, d_k_scalars_ptr: int, n: int) -> int:
        h = C.c_uint64()
        self._check(self._lib.h2agg_bases_generate(self._ctx, d_k_scalars_ptr, n, C.byref(h)))
        return h.value

    def bases_precompute(self, handle: int, window_bits: int = 0):
        """fixed-base levels for a resident table (SRS-style bases): later MSMs over it use one bucket set"""
        self._check(self._lib.h2agg_bases_precompute(self._ctx, handle, window_bits))

    def bases_download(self, handle: int, first: int, n: int) -> bytes:
        out = C.create_string_buffer(max(64 * n, 1))
        self._check(self._lib.h2agg_bases_download(self._ctx, handle, first, n, out))
        return out.raw[:64 * n]

    def bases_free(self, handle: int):
        self._check(self._lib.h2agg_bases_free(self._ctx, handle))

    def bases_fft(self, handle: int, k: int, inverse: bool = False) -> int:
        """the G1 Fourier transform of the first 2^k points of a resident table, as a new table; inverse=True is halo2's
        g_to_lagrange (ParamsKZG::downsize): out[i] = (1/n) sum_j w^(-ij) in[j]"""
        h = C.c_uint64()
        self._check(self._lib.h2agg_bases_fft(self._ctx, handle, k, int(bool(inverse)), C.byref(h)))
        return h.value

    # ------------------------------------------------------------------ Fr prover steps: shared argument handling
    @staticmethod
    def _hostptr(data):
        return C.cast(C.c_char_p(bytes(data)), C.c_void_p)

    def _in_place_or_new(self, data, call):
        """call(src, dst) -> the library's status.  A bytearray is transformed in place and returned; anything else is read
        as bytes and gives a new bytes object."""
        if isinstance(data, bytearray):
            buf = (C.c_char * len(data)).from_buffer(data)
            self._check(call(C.addressof(buf), C.addressof(buf)))
            return data
        out = C.create_string_buffer(max(len(data), 1))
        self._check(call(self._hostptr(data), out))
        return out.raw[:len(data)]

    @staticmethod
    def _need32(**named):
        for name, v in named.items():
            _need(v, 32, name)

    @staticmethod
    def _z_buffers(u: int):
        """(out, last) of a synchronous product call: z[0 .. u] and z[u]"""
        return C.create_string_buffer(32 * (max(u, 0) + 1)), C.create_string_buffer(32)

    def fr_fft(self, data, k: int, inverse: bool = False, shift: Optional[bytes] = None) -> bytes:
        """the Fourier transform over Fr of 2^k canonical 32-byte elements (h2agg_fr_fft): best_fft, or with inverse=True the
        inverse transform with its 1/n; shift=s transforms s^j * in[j] (forward) / multiplies out[j] by s^-j (inverse).  A
        bytearray is transformed in place and returned; bytes give a new bytes object."""
        if 0 <= k <= FR_FFT_MAX_K:   # (a larger k is refused by the library before it touches a buffer)
            _need(data, 32 << k, "data")
        if shift is not None:
            _need(shift, 32, "shift")
        return self._in_place_or_new(
            data, lambda src, dst: self._lib.h2agg_fr_fft(self._ctx, src, k, int(bool(inverse)), shift, dst))

    def fr_fft_batch(self, data, k: int, inverse: bool = False, shift: Optional[bytes] = None) -> bytes:
        """fr_fft of every column of a slab [m][2^k] in one call (h2agg_fr_fft_batch): m = len(data) / (32 * 2^k), column j of
        the result is fr_fft of column j.  A bytearray is transformed in place and returned; bytes give a new bytes object."""
        m = self._slab(data, k)
        if shift is not None:
            _need(shift, 32, "shift")
        return self._in_place_or_new(
            data, lambda src, dst: self._lib.h2agg_fr_fft_batch(self._ctx, src, m, k, int(bool(inverse)), shift, dst))

    def fr_fft_device(self, d_in_ptr: int, k: int, inverse: bool, shift: Optional[bytes], d_out_ptr: int):
        """h2agg_fr_fft_device: 2^k elements in device memory, queued on the context's stream (no synchronisation);
        d_out_ptr == d_in_ptr is allowed"""
        if shift is not None:
            _need(shift, 32, "shift")
        self._check(self._lib.h2agg_fr_fft_device(self._ctx, d_in_ptr, k, int(bool(inverse)), shift, d_out_ptr))

    # ------------------------------------------------------------------ KZG openings
    @staticmethod
    def _queries(queries, points: bytes):
        """[(poly, point), ...] -> the uint32 pairs of the C ABI; points: npoints x 32 bytes"""
        _need(points, 32 * (len(points) // 32), "points")
        flat = [int(x) for q in queries for x in q]
        if len(flat) != 2 * len(queries) or any(x < 0 or x >= 1 << 32 for x in flat):
            raise ValueError("queries must be (polynomial index, point index) pairs of 32-bit values")
        return (C.c_uint32 * max(len(flat), 1))(*flat), len(queries), len(points) // 32

    def _slab(self, polys, k: int):
        if not 0 <= k <= FR_FFT_MAX_K:   # (refused by the library before it touches a buffer)
            return 1
        _need(polys, (32 << k) * (len(polys) // (32 << k)), "polys")
        return len(polys) // (32 << k)

    def fr_poly_eval(self, polys: bytes, k: int, queries, points: bytes) -> bytes:
        """h2agg_fr_poly_eval: polys = a slab [npoly][2^k] of canonical coefficients, queries = [(poly, point), ...] into it
        and into points (npoints x 32 bytes) -> the nq values, 32 bytes each, in query order"""
        npoly = self._slab(polys, k)
        qs, nq, npoints = self._queries(queries, points)
        out = C.create_string_buffer(max(32 * nq, 1))
        self._check(self._lib.h2agg_fr_poly_eval(self._ctx, self._hostptr(polys), npoly, k, qs, nq, points, npoints, out))
        return out.raw[:32 * nq]

    def fr_poly_eval_device(self, d_polys_ptr: int, npoly: int, k: int, queries, points: bytes) -> bytes:
        """h2agg_fr_poly_eval_device: as fr_poly_eval over a slab already in device memory; synchronous"""
        qs, nq, npoints = self._queries(queries, points)
        out = C.create_string_buffer(max(32 * nq, 1))
        self._check(self._lib.h2agg_fr_poly_eval_device(self._ctx, d_polys_ptr, npoly, k, qs, nq, points, npoints, out))
        return out.raw[:32 * nq]

    def fr_poly_divide(self, coeffs, k: int, z: bytes):
        """h2agg_fr_poly_divide: 2^k coefficients -> (the 2^k coefficients of the quotient by (X - z), zero on top; a(z)).
        A bytearray is divided in place and returned; bytes give a new bytes object."""
        if 0 <= k <= FR_FFT_MAX_K:
            _need(coeffs, 32 << k, "coeffs")
        _need(z, 32, "z")
        rem = C.create_string_buffer(32)
        quot = self._in_place_or_new(coeffs, lambda src, dst: self._lib.h2agg_fr_poly_divide(self._ctx, src, k, z, dst, rem))
        return quot, rem.raw

    def fr_poly_divide_device(self, d_poly_ptr: int, k: int, z: bytes, d_quot_ptr: int, d_rem_ptr: Optional[int] = None):
        """h2agg_fr_poly_divide_device: device memory in and out, queued on the context's stream (no synchronisation);
        d_quot_ptr == d_poly_ptr is allowed; d_rem_ptr: 32 bytes of device memory, or None"""
        _need(z, 32, "z")
        self._check(self._lib.h2agg_fr_poly_divide_device(self._ctx, d_poly_ptr, k, z, d_quot_ptr, d_rem_ptr))

    def _multiopen(self, fn, g_handle: int, polys_arg, npoly: int, k: int, queries, points: bytes, v: bytes):
        _need(v, 32, "v")
        qs, nq, npoints = self._queries(queries, points)
        cap = max(min(nq, npoints), 1)
        w, gp, ng = C.create_string_buffer(64 * cap), (C.c_uint32 * cap)(), C.c_size_t()
        self._check(fn(self._ctx, g_handle, polys_arg, npoly, k, qs, nq, points, npoints, v, w, gp, C.byref(ng)))
        return list(gp[:ng.value]), [w.raw[64 * g:64 * g + 64] for g in range(ng.value)]

    def kzg_multiopen(self, g_handle: int, polys: bytes, k: int, queries, points: bytes, v: bytes):
        """h2agg_kzg_multiopen: the GWC opening of queries [(poly, point), ...] over a host slab [npoly][2^k] -> (the point
        index of every group in first-seen order, the canonical affine W of every group)"""
        npoly = self._slab(polys, k)
        return self._multiopen(self._lib.h2agg_kzg_multiopen, g_handle, self._hostptr(polys), npoly, k, queries, points, v)

    def kzg_multiopen_device(self, g_handle: int, d_polys_ptr: int, npoly: int, k: int, queries, points: bytes, v: bytes):
        """h2agg_kzg_multiopen_device: as kzg_multiopen over a slab already in device memory"""
        return self._multiopen(self._lib.h2agg_kzg_multiopen_device, g_handle, d_polys_ptr, npoly, k, queries, points, v)

    def kzg_shplonk_begin(self, g_handle: int, polys: bytes, k: int, queries, points: bytes, evals: bytes, y: bytes, v: bytes):
        """h2agg_kzg_shplonk_begin: round 1 of the Shplonk opening of queries [(poly, point), ...] over a host slab
        [npoly][2^k], evals = the nq values in query order -> (the canonical affine H1, the object for kzg_shplonk_finish).
        The object holds device memory of this context: kzg_shplonk_destroy it (before the context closes)."""
        npoly = self._slab(polys, k)
        qs, nq, npoints = self._queries(queries, points)
        _need(evals, 32 * nq, "evals")
        _need(y, 32, "y")
        _need(v, 32, "v")
        h1, obj = C.create_string_buffer(64), C.c_void_p()
        self._check(self._lib.h2agg_kzg_shplonk_begin(self._ctx, g_handle, self._hostptr(polys), npoly, k, qs, nq, points, npoints,
                                                      evals, y, v, h1, C.byref(obj)))
        return h1.raw, obj

    def kzg_shplonk_finish(self, obj, u: bytes) -> bytes:
        """h2agg_kzg_shplonk_finish: round 2 for the challenge u -> the canonical affine H2; may be called again"""
        _need(u, 32, "u")
        if not obj:
            raise ValueError("obj must be an object of kzg_shplonk_begin that has not been destroyed")
        h2 = C.create_string_buffer(64)
        self._check(self._lib.h2agg_kzg_shplonk_finish(obj, u, h2))
        return h2.raw

    def kzg_shplonk_destroy(self, obj):
        """h2agg_kzg_shplonk_destroy: frees the object; the handle is cleared, a second call does nothing"""
        if obj:
            self._lib.h2agg_kzg_shplonk_destroy(obj)
            obj.value = None

    # ------------------------------------------------------------------ grand products
    def _column(self, data, k: int, u: int, what: str, cols: int = 1):
        """a column slab [cols][2^k]; sizes are checked only where the library would go on to read the buffer"""
        if 0 <= k <= FR_FFT_MAX_K and 0 <= u < (1 << k) and 1 <= cols <= FR_PROD_MAX_COLUMNS:
            _need(data, (32 << k) * cols, what)
        return self._hostptr(data)

    def fr_batch_invert(self, data):
        """h2agg_fr_batch_invert: n canonical elements -> their inverses, 0 for 0 (ff::BatchInvert).  A bytearray is inverted
        in place and returned; bytes give a new bytes object."""
        n = len(data) // 32
        _need(data, 32 * n, "data")
        return self._in_place_or_new(data, lambda src, dst: self._lib.h2agg_fr_batch_invert(self._ctx, src, n, dst))

    def fr_batch_invert_device(self, d_in_ptr: int, n: int, d_out_ptr: int):
        """h2agg_fr_batch_invert_device: n elements in device memory, queued on the context's stream (no synchronisation);
        d_out_ptr == d_in_ptr is allowed"""
        self._check(self._lib.h2agg_fr_batch_invert_device(self._ctx, d_in_ptr, n, d_out_ptr))

    def fr_grand_product(self, num: bytes, den: Optional[bytes], k: int, u: int, init: bytes):
        """h2agg_fr_grand_product: -> (out[0 .. u] as 32 * (u + 1) bytes, out[u]); num (and den, or None) hold u elements"""
        _need(init, 32, "init")
        if 0 <= k <= FR_FFT_MAX_K and 0 <= u < (1 << k):
            _need(num, 32 * u, "num")
            if den is not None:
                _need(den, 32 * u, "den")
        out, last = self._z_buffers(u)
        self._check(self._lib.h2agg_fr_grand_product(self._ctx, self._hostptr(num), None if den is None else self._hostptr(den),
                                                     k, u, init, out, last))
        return out.raw, last.raw

    def fr_grand_product_device(self, d_num_ptr: int, d_den_ptr: Optional[int], k: int, u: int, init: bytes, d_out_ptr: int,
                                d_last_ptr: Optional[int] = None):
        """h2agg_fr_grand_product_device: device memory in and out, queued on the context's stream (no synchronisation);
        d_out_ptr may alias d_num_ptr; d_den_ptr and d_last_ptr may be None"""
        _need(init, 32, "init")
        self._check(self._lib.h2agg_fr_grand_product_device(self._ctx, d_num_ptr, d_den_ptr, k, u, init, d_out_ptr, d_last_ptr))

    def permutation_product(self, values: bytes, sigmas: bytes, m: int, k: int, u: int, beta: bytes, gamma: bytes, delta: bytes,
                            delta_first: bytes, init: bytes):
        """h2agg_permutation_product: one permutation set of m columns (slabs [m][2^k]) -> (z[0 .. u], z[u])"""
        self._need32(beta=beta, gamma=gamma, delta=delta, delta_first=delta_first, init=init)
        out, last = self._z_buffers(u)
        self._check(self._lib.h2agg_permutation_product(self._ctx, self._column(values, k, u, "values", m),
                                                        self._column(sigmas, k, u, "sigmas", m), m, k, u, beta, gamma, delta,
                                                        delta_first, init, out, last))
        return out.raw, last.raw

    def permutation_product_device(self, d_values_ptr: int, d_sigmas_ptr: int, m: int, k: int, u: int, beta: bytes, gamma: bytes,
                                   delta: bytes, delta_first: bytes, init: bytes, d_out_ptr: int, d_last_ptr: Optional[int] = None):
        """h2agg_permutation_product_device: slabs and z in device memory, queued on the context's stream (no synchronisation)"""
        self._need32(beta=beta, gamma=gamma, delta=delta, delta_first=delta_first, init=init)
        self._check(self._lib.h2agg_permutation_product_device(self._ctx, d_values_ptr, d_sigmas_ptr, m, k, u, beta, gamma, delta,
                                                               delta_first, init, d_out_ptr, d_last_ptr))

    def lookup_product(self, a: bytes, s: bytes, ap: bytes, sp: bytes, k: int, u: int, beta: bytes, gamma: bytes):
        """h2agg_lookup_product: compressed input, table and their permuted forms (2^k rows each) -> (z[0 .. u], z[u])"""
        self._need32(beta=beta, gamma=gamma)
        out, last = self._z_buffers(u)
        cols = [self._column(x, k, u, what) for x, what in ((a, "a"), (s, "s"), (ap, "ap"), (sp, "sp"))]
        self._check(self._lib.h2agg_lookup_product(self._ctx, *cols, k, u, beta, gamma, out, last))
        return out.raw, last.raw

    def lookup_product_device(self, d_a_ptr: int, d_s_ptr: int, d_ap_ptr: int, d_sp_ptr: int, k: int, u: int, beta: bytes,
                              gamma: bytes, d_out_ptr: int, d_last_ptr: Optional[int] = None):
        """h2agg_lookup_product_device: columns and z in device memory, queued on the context's stream (no synchronisation)"""
        self._need32(beta=beta, gamma=gamma)
        self._check(self._lib.h2agg_lookup_product_device(self._ctx, d_a_ptr, d_s_ptr, d_ap_ptr, d_sp_ptr, k, u, beta, gamma,
                                                          d_out_ptr, d_last_ptr))

    # ------------------------------------------------------------------ lookup argument: compression, permutation
    def lookup_permute(self, a: bytes, s: bytes, k: int, u: int):
        """h2agg_lookup_permute: the first u rows of the compressed input and table -> (ap, sp), 32 * u bytes each
        (permute_expression_pair); a and s hold at least u elements, only those are read"""
        if 0 <= k <= FR_FFT_MAX_K and 0 <= u < (1 << k):
            for x, what in ((a, "a"), (s, "s")):
                if x is None or len(x) < 32 * u or len(x) % 32:
                    raise ValueError("%s must hold at least %d elements of 32 bytes" % (what, u))
        ap, sp = C.create_string_buffer(32 * max(u, 1)), C.create_string_buffer(32 * max(u, 1))
        self._check(self._lib.h2agg_lookup_permute(self._ctx, self._hostptr(a), self._hostptr(s), k, u, ap, sp))
        return ap.raw[:32 * max(u, 0)], sp.raw[:32 * max(u, 0)]

    def lookup_permute_device(self, d_a_ptr: int, d_s_ptr: int, k: int, u: int, d_ap_ptr: int, d_sp_ptr: int):
        """h2agg_lookup_permute_device: columns in device memory, queued on the context's stream (no synchronisation); rows
        from u up of d_ap / d_sp are left alone; d_ap / d_sp must not overlap d_a, d_s or each other"""
        self._check(self._lib.h2agg_lookup_permute_device(self._ctx, d_a_ptr, d_s_ptr, k, u, d_ap_ptr, d_sp_ptr))

    # ------------------------------------------------------------------ lookup argument, batched
    def lookup_configure(self, batch_chunk: int):
        """h2agg_lookup_configure: at most batch_chunk lookups per set of launches of a batch (0 = the default rule)"""
        self._check(self._lib.h2agg_lookup_configure(self._ctx, int(batch_chunk)))

    @staticmethod
    def lookup_chunk_rule(u: int, batch_chunk: int = 0) -> int:
        """h2agg_lookup_chunk_rule: the lookups per chunk at u rows under lookup_configure(batch_chunk); host arithmetic"""
        return int(load_library().h2agg_lookup_chunk_rule(int(u), int(batch_chunk)))

    @staticmethod
    def _batch_slab(x, count: int, k: int, what: str):
        if 0 <= k <= FR_FFT_MAX_K and 1 <= count <= 65535:
            _need(x, (32 << k) * count, what)

    def lookup_batch_permute(self, a: bytes, s: bytes, count: int, k: int, u: int, ap=None, sp=None):
        """h2agg_lookup_batch_permute: slabs [count][2^k] -> (ap, sp, status): slabs whose rows from u up are what ap / sp (the
        caller's pre-filled slabs, or zero) held, and the per-lookup status words.  Raises the error of the lowest-numbered
        failing lookup, with the slabs and the words in the exception's .partial"""
        for x, what in ((a, "a"), (s, "s")):
            self._batch_slab(x, count, k, what)
        size = (32 << k) * count if 0 <= k <= FR_FFT_MAX_K and 1 <= count <= 65535 else 32
        outs = []
        for x, what in ((ap, "ap"), (sp, "sp")):
            if x is not None:
                _need(x, size, what)
            outs.append(C.create_string_buffer(bytes(x), size) if x is not None else C.create_string_buffer(size))
        status = (C.c_uint32 * max(count, 1))()
        rc = self._lib.h2agg_lookup_batch_permute(self._ctx, self._hostptr(a), self._hostptr(s), count, k, u, outs[0], outs[1],
                                                  status)
        result = (outs[0].raw, outs[1].raw, list(status)[:max(count, 0)])
        try:
            self._check(rc)
        except H2AggError as e:
            e.partial = result
            raise
        return result

    def lookup_batch_product(self, a: bytes, s: bytes, ap: bytes, sp: bytes, count: int, k: int, u: int, beta: bytes,
                             gamma: bytes, z=None):
        """h2agg_lookup_batch_product: slabs [count][2^k] -> (z, last): the slab whose rows from u + 1 up are what z (the
        caller's pre-filled slab, or zero) held, and the list of z[j][u]"""
        self._need32(beta=beta, gamma=gamma)
        for x, what in ((a, "a"), (s, "s"), (ap, "ap"), (sp, "sp")):
            self._batch_slab(x, count, k, what)
        size = (32 << k) * count if 0 <= k <= FR_FFT_MAX_K and 1 <= count <= 65535 else 32
        if z is not None:
            _need(z, size, "z")
        out = C.create_string_buffer(bytes(z), size) if z is not None else C.create_string_buffer(size)
        last = C.create_string_buffer(32 * max(count, 1))
        self._check(self._lib.h2agg_lookup_batch_product(self._ctx, self._hostptr(a), self._hostptr(s), self._hostptr(ap),
                                                         self._hostptr(sp), count, k, u, beta, gamma, out, last))
        return out.raw, [last.raw[32 * j:32 * j + 32] for j in range(count)]

    def lookup_store_permute(self, a: int, afirst: int, s: int, sfirst: int, count: int, u: int, ap: int, apfirst: int, sp: int,
                             spfirst: int, want_status: bool = True):
        """h2agg_lookup_store_permute over column-store handles.  want_status: synchronous, -> the status words (an error is
        raised with them in .partial); else queued with no synchronisation -> None"""
        status = (C.c_uint32 * max(count, 1))() if want_status else None
        rc = self._lib.h2agg_lookup_store_permute(self._ctx, a, afirst, s, sfirst, count, u, ap, apfirst, sp, spfirst, status)
        result = list(status)[:max(count, 0)] if want_status else None
        try:
            self._check(rc)
        except H2AggError as e:
            e.partial = result
            raise
        return result

    def lookup_store_product(self, a: int, afirst: int, s: int, sfirst: int, ap: int, apfirst: int, sp: int, spfirst: int,
                             count: int, u: int, beta: bytes, gamma: bytes, z: int, zfirst: int, want_last: bool = True):
        """h2agg_lookup_store_product over column-store handles.  want_last: synchronous, -> the list of z[j][u]; else queued
        with no synchronisation -> None"""
        self._need32(beta=beta, gamma=gamma)
        last = C.create_string_buffer(32 * max(count, 1)) if want_last else None
        self._check(self._lib.h2agg_lookup_store_product(self._ctx, a, afirst, s, sfirst, ap, apfirst, sp, spfirst, count, u, beta,
                                                         gamma, z, zfirst, last))
        return [last.raw[32 * j:32 * j + 32] for j in range(count)] if want_last else None

    def fr_columns_compress(self, cols: bytes, m: int, k: int, theta: bytes) -> bytes:
        """h2agg_fr_columns_compress: a slab [m][2^k] -> out[i] = sum_j theta^(m - 1 - j) cols[j][i], 2^k elements"""
        self._need32(theta=theta)
        if not (0 <= k <= FR_FFT_MAX_K and m >= 1):
            raise H2AggError(ERR_INVALID, "fr_columns_compress: k must be 0 .. %d and m >= 1" % FR_FFT_MAX_K)
        _need(cols, (32 << k) * m, "cols")       # (the library refuses an m above its limit before it reads cols)
        out = C.create_string_buffer(32 << k)
        self._check(self._lib.h2agg_fr_columns_compress(self._ctx, self._hostptr(cols), m, k, theta, out))
        return out.raw

    def fr_columns_compress_device(self, d_cols_ptr: int, m: int, k: int, theta: bytes, d_out_ptr: int):
        """h2agg_fr_columns_compress_device: slab and result in device memory, queued on the context's stream (no
        synchronisation); d_out_ptr may be one of the columns"""
        self._need32(theta=theta)
        self._check(self._lib.h2agg_fr_columns_compress_device(self._ctx, d_cols_ptr, m, k, theta, d_out_ptr))

    # ------------------------------------------------------------------ quotient polynomial
    def _slab_or_null(self, data):
        return None if data is None else self._hostptr(data)

    def _vk_slabs(self, vk, k: int, named):
        """host slabs of a key's columns: (data or None, count, name) -> pointers; where k is the key's, the library reads
        count * 2^k elements of each, so their sizes are checked here"""
        out = []
        for data, count, what in named:
            if data is not None and k == vk.shape["k"]:
                _need(data, (32 << k) * count, what)
            out.append(self._slab_or_null(data))
        return out

    @staticmethod
    def _vk_challenges(vk, challenges):
        if challenges is not None:
            _need(challenges, 32 * vk.shape["num_challenges"], "challenges")
        return challenges

    def vk_expressions_eval(self, vk, which: int, j: int, k: int, advice, fixed, instance, challenges,
                            fold: Optional[bytes] = None) -> bytes:
        """h2agg_vk_expressions_eval: expressions of the key `vk` (a verifier.VerifyingKey) on every row of host value slabs
        [columns][2^k] (None for a slab without columns; challenges: num_challenges x 32 bytes or None).  which = 0: the gate
        polynomials, 1 / 2: the input / table expressions of lookup j.  fold None -> the slab [expressions][2^k]; a 32-byte
        fold -> one column.  The sizes come from vk.shape."""
        sh = vk.shape
        if fold is not None:
            _need(fold, 32, "fold")
        m = sh["gate_polys"] if which == 0 else sh["lookups"][j][which - 1] if which in (1, 2) and 0 <= j < len(sh["lookups"]) else 0
        cols = 1 if fold is not None else m
        out = C.create_string_buffer(max((32 << sh["k"]) * cols, 1))   # (the library writes only when k is the key's)
        slabs = self._vk_slabs(vk, k, ((advice, sh["num_advice"], "advice"), (fixed, sh["num_fixed"], "fixed"),
                                       (instance, sh["num_instance"], "instance")))
        self._check(self._lib.h2agg_vk_expressions_eval(self._ctx, vk._vk, which, j, k, *slabs, self._vk_challenges(vk, challenges),
                                                        fold, out))
        return out.raw[:(32 << sh["k"]) * cols]

    def vk_expressions_eval_device(self, vk, which: int, j: int, k: int, d_advice_ptr, d_fixed_ptr, d_instance_ptr, challenges,
                                   fold: Optional[bytes], d_out_ptr):
        """h2agg_vk_expressions_eval_device: slabs and result in device memory, queued on the context's stream (no
        synchronisation)"""
        if fold is not None:
            _need(fold, 32, "fold")
        self._check(self._lib.h2agg_vk_expressions_eval_device(self._ctx, vk._vk, which, j, k, d_advice_ptr, d_fixed_ptr,
                                                               d_instance_ptr, challenges, fold, d_out_ptr))

    def quotient(self, vk, advice, fixed, instance, sigma, perm_z, lookup_z, lookup_ap, lookup_sp, challenges, theta: bytes,
                 beta: bytes, gamma: bytes, y: bytes, delta: bytes) -> bytes:
        """h2agg_quotient: coefficient slabs [polynomials][2^k] on the host (None for a slab without polynomials) -> the slab
        [degree - 1][2^k] of h's pieces.  The sizes come from vk.shape."""
        self._need32(theta=theta, beta=beta, gamma=gamma, y=y, delta=delta)
        sh = vk.shape
        k, pieces, nl = sh["k"], sh["degree"] - 1, len(sh["lookups"])
        nsets = -(-sh["num_permutation_columns"] // (sh["degree"] - 2))
        slabs = self._vk_slabs(vk, k, ((advice, sh["num_advice"], "advice"), (fixed, sh["num_fixed"], "fixed"),
                                       (instance, sh["num_instance"], "instance"), (sigma, sh["num_permutation_columns"], "sigma"),
                                       (perm_z, nsets, "perm_z"), (lookup_z, nl, "lookup_z"), (lookup_ap, nl, "lookup_ap"),
                                       (lookup_sp, nl, "lookup_sp")))
        if (pieces << k) > (1 << FR_FFT_MAX_K):   # (the library refuses it as well: the extended domain is 2^(k+e) >= pieces * 2^k)
            raise H2AggError(ERR_INVALID, "quotient: the host-buffer form takes extended domains <= 2^%d (quotient_device: <= 2^%d)"
                             % (FR_FFT_MAX_K, FR_QUOTIENT_MAX_K))
        out = C.create_string_buffer((32 << k) * pieces)
        self._check(self._lib.h2agg_quotient(self._ctx, vk._vk, *slabs, self._vk_challenges(vk, challenges), theta, beta, gamma, y,
                                             delta, out))
        return out.raw

    def quotient_device(self, vk, d_advice_ptr, d_fixed_ptr, d_instance_ptr, d_sigma_ptr, d_perm_z_ptr, d_lookup_z_ptr,
                        d_lookup_ap_ptr, d_lookup_sp_ptr, challenges, theta: bytes, beta: bytes, gamma: bytes, y: bytes,
                        delta: bytes, d_h_ptr):
        """h2agg_quotient_device: coefficient slabs and the pieces in device memory, queued on the context's stream (no
        synchronisation, no read-back)"""
        self._need32(theta=theta, beta=beta, gamma=gamma, y=y, delta=delta)
        self._check(self._lib.h2agg_quotient_device(self._ctx, vk._vk, d_advice_ptr, d_fixed_ptr, d_instance_ptr, d_sigma_ptr,
                                                    d_perm_z_ptr, d_lookup_z_ptr, d_lookup_ap_ptr, d_lookup_sp_ptr, challenges,
                                                    theta, beta, gamma, y, delta, d_h_ptr))

    def quotient_configure(self, split: int):
        """h2agg_quotient_configure: 1 = every quotient of this context takes the coset-split ending (per-coset inverse
        transforms of size 2^k and k_qe_cross_cosets), 0 = only where the extended domain is above 2^24 (the default)"""
        self._check(self._lib.h2agg_quotient_configure(self._ctx, int(split)))

    def quotient_work_bytes(self, vk) -> int:
        """h2agg_quotient_work_bytes: the device work memory a quotient call of this key holds in the context (the coset's value
        slab, the Lagrange rows, the fold columns, the extended evaluations or the cosets' inverse transforms, the transforms'
        work array), on the route the key takes by its size; a key the quotient refuses: ERR_INVALID"""
        out = C.c_size_t()
        self._check(self._lib.h2agg_quotient_work_bytes(vk._vk, C.byref(out)))
        return out.value

    # ------------------------------------------------------------------ keys
    def permutation_sigmas(self, mapping, m: int, k: int, usable: int, delta: bytes, lagrange: bool = True, coeff: bool = True):
        """h2agg_permutation_sigmas: the mapping of a permutation over m columns of 2^k rows (2 * m * 2^k words: bytes,
        array('I') or a ctypes array, as permutation_assembly returns it) -> (lagrange, coeff): the sigma columns as slabs
        [m][2^k] in Lagrange and in coefficient form.  lagrange=False / coeff=False leaves that output out (None)."""
        _need(delta, 32, "delta")
        ok = _perm_shape_ok(m, k, usable)
        words = _words(mapping, 2 * m << k, "mapping") if ok else (C.c_uint32 * 1)()
        size = (32 * m << k) if ok else 1
        lag = C.create_string_buffer(size) if lagrange else None
        co = C.create_string_buffer(size) if coeff else None
        self._check(self._lib.h2agg_permutation_sigmas(self._ctx, words, m, k, usable, delta, lag, co))
        return (None if lag is None else lag.raw[:size], None if co is None else co.raw[:size])

    def commit_columns(self, handle: int, columns, k: int) -> List[bytes]:
        """h2agg_commit_columns: a slab [m][2^k] of canonical scalars -> the m commitments sum_i columns[j][i] * table[i] as
        64-byte canonical affine points (the identity: 64 zero bytes), through one staging and the batched MSM"""
        m = self._slab(columns, k) if 0 <= k <= FR_FFT_MAX_K else 1
        out = C.create_string_buffer(max(64 * m, 1))
        self._check(self._lib.h2agg_commit_columns(self._ctx, handle, self._hostptr(columns), m, k, out))
        return [out.raw[64 * j:64 * j + 64] for j in range(m)]

    # ------------------------------------------------------------------ witness check
    def witness_check_layout(self, vk):
        """h2agg_witness_check_layout: -> (gate polynomials, permutation columns, lookups) of the key: the constraints of
        witness_check, in that order"""
        g, p, l = C.c_size_t(), C.c_size_t(), C.c_size_t()
        self._check(self._lib.h2agg_witness_check_layout(vk._vk, C.byref(g), C.byref(p), C.byref(l)))
        return g.value, p.value, l.value

    def witness_check(self, vk, what: int, advice, fixed, instance, challenges, theta: Optional[bytes], mapping,
                      max_rows: int = 16, want_rows: bool = True):
        """h2agg_witness_check: Lagrange value slabs [columns][2^k] on the host (None for a slab without columns), the
        permutation's mapping (2 * P * 2^k words as permutation_assembly returns it, or None) and theta (or None) ->
        (counts, first_rows, rows, total): per constraint (gate polynomials, then permutation columns, then lookups) the
        number of failing rows, the lowest one (0xFFFFFFFF: none) and the lowest max_rows of them (rows[c]: a list of
        max_rows words, 0xFFFFFFFF behind the last; None with want_rows=False), and the sum of the counts.  `what`: WC_GATES |
        WC_PERMUTATION | WC_LOOKUPS.  The sizes come from vk.shape."""
        sh = vk.shape
        k = sh["k"]
        ncons = sh["gate_polys"] + sh["num_permutation_columns"] + len(sh["lookups"])
        if theta is not None:
            _need(theta, 32, "theta")
        if max_rows < 0:
            raise ValueError("max_rows must be >= 0")
        slabs = self._vk_slabs(vk, k, ((advice, sh["num_advice"], "advice"), (fixed, sh["num_fixed"], "fixed"),
                                       (instance, sh["num_instance"], "instance")))
        words = None if mapping is None else _words(mapping, 2 * sh["num_permutation_columns"] << k, "mapping")
        counts, first = (C.c_uint32 * max(ncons, 1))(), (C.c_uint32 * max(ncons, 1))()
        rows = (C.c_uint32 * max(ncons * max_rows, 1))() if want_rows else None
        total = C.c_uint64()
        self._check(self._lib.h2agg_witness_check(self._ctx, vk._vk, what, *slabs, self._vk_challenges(vk, challenges), theta, words,
                                                  max_rows, counts, first, rows, C.byref(total)))
        lines = None if rows is None else [list(rows[c * max_rows:(c + 1) * max_rows]) for c in range(ncons)]
        return list(counts[:ncons]), list(first[:ncons]), lines, total.value

    # ------------------------------------------------------------------ proving key on the device
    def _pk_create(self, fn, vk, fixed, sigma, forms: int):
        pk = C.c_void_p()
        self._check(fn(self._ctx, vk._vk, fixed, sigma, forms, C.byref(pk)))
        return pk

    def pk_create(self, vk, fixed, sigma, forms: int = PK_COSETS):
        """h2agg_pk_create: the host slabs fixed[num_fixed][2^k] and sigma[num_permutation_columns][2^k] in Lagrange form (None
        for a slab without columns) -> the object (pass it to pk_quotient; free it with pk_destroy before the key and the
        engine go).  Synchronous.  forms: 0 or PK_COSETS.  The sizes come from vk.shape."""
        sh = vk.shape
        slabs = self._vk_slabs(vk, sh["k"], ((fixed, sh["num_fixed"], "fixed"), (sigma, sh["num_permutation_columns"], "sigma")))
        return self._pk_create(self._lib.h2agg_pk_create, vk, *slabs, forms)

    def pk_create_resident(self, vk, d_fixed_ptr, d_sigma_ptr, forms: int = PK_COSETS):
        """h2agg_pk_create_resident: the same from slabs in device memory (not written); synchronous"""
        return self._pk_create(self._lib.h2agg_pk_create_resident, vk, d_fixed_ptr, d_sigma_ptr, forms)

    def pk_bytes(self, vk, forms: int = PK_COSETS) -> int:
        """h2agg_pk_bytes: the device memory a proving key of this verifying key holds with these forms"""
        out = C.c_size_t()
        self._check(self._lib.h2agg_pk_bytes(vk._vk, forms, C.byref(out)))
        return out.value

    def pk_info(self, pk) -> dict:
        """h2agg_pk_info: -> {"k", "e", "num_fixed", "num_permutation_columns", "forms", "bytes"}"""
        k, e, forms = C.c_uint(), C.c_uint(), C.c_uint()
        nf, np_, nbytes = C.c_size_t(), C.c_size_t(), C.c_size_t()
        self._check(self._lib.h2agg_pk_info(pk, C.byref(k), C.byref(e), C.byref(nf), C.byref(np_), C.byref(forms), C.byref(nbytes)))
        return {"k": k.value, "e": e.value, "num_fixed": nf.value, "num_permutation_columns": np_.value, "forms": forms.value,
                "bytes": nbytes.value}

    def pk_ptr(self, pk, which: int, coset: int = 0):
        """h2agg_pk_ptr: -> (the device address of the form `which` (PK_*), None for a form without columns; its columns).
        Read-only; valid until the object goes."""
        p, cols = C.c_void_p(), C.c_size_t()
        self._check(self._lib.h2agg_pk_ptr(pk, which, coset, C.byref(p), C.byref(cols)))
        return p.value, cols.value

    def pk_quotient(self, pk, d_advice_ptr, d_instance_ptr, d_perm_z_ptr, d_lookup_z_ptr, d_lookup_ap_ptr, d_lookup_sp_ptr,
                    challenges, theta: bytes, beta: bytes, gamma: bytes, y: bytes, delta: bytes, d_h_ptr):
        """h2agg_pk_quotient: quotient_device with the fixed and sigma polynomials (and, with PK_COSETS, their values on every
        coset) taken from the proving key; queued on the context's stream (no synchronisation, no read-back)"""
        self._need32(theta=theta, beta=beta, gamma=gamma, y=y, delta=delta)
        self._check(self._lib.h2agg_pk_quotient(self._ctx, pk, d_advice_ptr, d_instance_ptr, d_perm_z_ptr, d_lookup_z_ptr,
                                                d_lookup_ap_ptr, d_lookup_sp_ptr, challenges, theta, beta, gamma, y, delta, d_h_ptr))

    def pk_quotient_work_bytes(self, pk) -> int:
        """h2agg_pk_quotient_work_bytes: the device work memory a pk_quotient call of this object holds in the context"""
        out = C.c_size_t()
        self._check(self._lib.h2agg_pk_quotient_work_bytes(pk, C.byref(out)))
        return out.value

    def pk_destroy(self, pk):
        """h2agg_pk_destroy: waits for the context's stream and frees the object; the handle is cleared, a second call does
        nothing"""
        if pk:
            self._lib.h2agg_pk_destroy(pk)
            pk.value = None

    # ------------------------------------------------------------------ Fr column stores
    def columns_create(self, m: int, k: int) -> int:
        """h2agg_columns_create: a zero-filled slab [m][2^k] of Fr in device memory that the context owns -> its handle"""
        h = C.c_uint64()
        self._check(self._lib.h2agg_columns_create(self._ctx, m, k, C.byref(h)))
        return h.value

    def columns_destroy(self, handle: int):
        self._check(self._lib.h2agg_columns_destroy(self._ctx, handle))

    def columns_info(self, handle: int):
        """h2agg_columns_info: -> (m, k)"""
        m, k = C.c_size_t(), C.c_uint()
        self._check(self._lib.h2agg_columns_info(self._ctx, handle, C.byref(m), C.byref(k)))
        return m.value, k.value

    def columns_write(self, handle: int, first: int, data, count: Optional[int] = None):
        """h2agg_columns_write: data = whole columns (32 * 2^k bytes each) to columns first, first + 1, ... of the store, or the
        address of a host buffer (e.g. from host_alloc) together with count; synchronous; an element >= r raises
        H2AggError(ERR_NONCANONICAL)"""
        if isinstance(data, int):
            self._check(self._lib.h2agg_columns_write(self._ctx, handle, first, count, C.c_void_p(data)))
            return
        _m, k = self.columns_info(handle)
        count = len(data) // (32 << k)
        _need(data, (32 << k) * count, "data")
        self._check(self._lib.h2agg_columns_write(self._ctx, handle, first, count, self._hostptr(data)))

    def columns_read(self, handle: int, first: int, count: int) -> bytes:
        """h2agg_columns_read: columns first .. first + count - 1 of the store as bytes; synchronous"""
        m, k = self.columns_info(handle)
        ok = count >= 1 and 0 <= first and first + count <= m   # (the library refuses the others before it writes)
        out = C.create_string_buffer((32 << k) * count if ok else 1)
        self._check(self._lib.h2agg_columns_read(self._ctx, handle, first, count, out))
        return out.raw[:(32 << k) * count]

    def columns_ptr(self, handle: int, first: int = 0) -> int:
        """h2agg_columns_ptr: the device address of column `first`, for the _device entry points; valid until the store goes"""
        p = C.c_void_p()
        self._check(self._lib.h2agg_columns_ptr(self._ctx, handle, first, C.byref(p)))
        return p.value

    def columns_move(self, src: int, sfirst: int, dst: int, dfirst: int, count: int, rotation: int = 0):
        """h2agg_columns_move: dst[dfirst + j][i] = src[sfirst + j][(i + rotation) mod 2^k], j < count; queued"""
        if not -(1 << 31) <= rotation < (1 << 31):
            raise ValueError("rotation must be an int32")
        self._check(self._lib.h2agg_columns_move(self._ctx, src, sfirst, dst, dfirst, count, rotation))

    def columns_fft(self, src: int, sfirst: int, dst: int, dfirst: int, count: int, inverse: bool = False,
                    shift: Optional[bytes] = None):
        """h2agg_columns_fft: fr_fft_batch of `count` columns of a store into a store (the same range: in place); queued"""
        if shift is not None:
            _need(shift, 32, "shift")
        self._check(self._lib.h2agg_columns_fft(self._ctx, src, sfirst, dst, dfirst, count, int(bool(inverse)), shift))

    def columns_commit(self, bases_handle: int, src: int, first: int, count: int) -> List[bytes]:
        """h2agg_columns_commit: commit_columns of `count` columns of a store -> canonical affine points, 64 bytes each"""
        out = C.create_string_buffer(64 * count if 0 < count < (1 << 32) else 1)
        self._check(self._lib.h2agg_columns_commit(self._ctx, bases_handle, src, first, count, out))
        return [out.raw[64 * j:64 * j + 64] for j in range(count)]

    def columns_sigmas(self, mapping, m: int, k: int, usable: int, delta: bytes, dst_lagrange: int = 0, lfirst: int = 0,
                       dst_coeff: int = 0, cfirst: int = 0):
        """h2agg_columns_sigmas: permutation_sigmas with the outputs in stores (a handle of 0: that output is not wanted)"""
        _need(delta, 32, "delta")
        words = _words(mapping, 2 * m << k, "mapping") if _perm_shape_ok(m, k, usable) else (C.c_uint32 * 1)()
        self._check(self._lib.h2agg_columns_sigmas(self._ctx, words, m, k, usable, delta, dst_lagrange, lfirst, dst_coeff, cfirst))

    def columns_witness_check(self, vk, what: int, advice, fixed, instance, challenges, theta: Optional[bytes], mapping,
                              max_rows: int = 16, want_rows: bool = True):
        """h2agg_columns_witness_check: witness_check with the slabs in stores: advice, fixed, instance are (handle, first
        column) pairs, or None where the key has no column of the kind -> (counts, first_rows, rows, total) as witness_check"""
        sh = vk.shape
        k = sh["k"]
        ncons = sh["gate_polys"] + sh["num_permutation_columns"] + len(sh["lookups"])
        if theta is not None:
            _need(theta, 32, "theta")
        if max_rows < 0:
            raise ValueError("max_rows must be >= 0")
        places = [x for pair in (advice, fixed, instance) for x in ((0, 0) if pair is None else (int(pair[0]), int(pair[1])))]
        words = None if mapping is None else _words(mapping, 2 * sh["num_permutation_columns"] << k, "mapping")
        counts, first = (C.c_uint32 * max(ncons, 1))(), (C.c_uint32 * max(ncons, 1))()
        rows = (C.c_uint32 * max(ncons * max_rows, 1))() if want_rows else None
        total = C.c_uint64()
        self._check(self._lib.h2agg_columns_witness_check(self._ctx, vk._vk, what, *places, self._vk_challenges(vk, challenges), theta,
                                                          words, max_rows, counts, first, rows, C.byref(total)))
        lines = None if rows is None else [list(rows[c * max_rows:(c + 1) * max_rows]) for c in range(ncons)]
        return list(counts[:ncons]), list(first[:ncons]), lines, total.value

    def columns_shplonk_begin(self, g_handle: int, src: int, first: int, npoly: int, queries, points: bytes, evals: bytes,
                              y: bytes, v: bytes):
        """h2agg_columns_shplonk_begin: kzg_shplonk_begin over npoly columns of a store -> (H1, the object for
        kzg_shplonk_finish / kzg_shplonk_destroy); the store is free again when the call returns"""
        qs, nq, npoints = self._queries(queries, points)
        _need(evals, 32 * nq, "evals")
        _need(y, 32, "y")
        _need(v, 32, "v")
        h1, obj = C.create_string_buffer(64), C.c_void_p()
        self._check(self._lib.h2agg_columns_shplonk_begin(self._ctx, g_handle, src, first, npoly, qs, nq, points, npoints, evals, y, v,
                                                          h1, C.byref(obj)))
        return h1.raw, obj

    def params_setup(self, k: int, s: bytes):
        """ParamsKZG::setup with the trapdoor `s` (32-byte LE, canonical) -> (g_handle, g_lagrange_handle), 2^k points each"""
        _need(s, 32, "s")
        g, gl = C.c_uint64(), C.c_uint64()
        self._check(self._lib.h2agg_params_setup(self._ctx, k, s, C.byref(g), C.byref(gl)))
        return g.value, gl.value

    def g2_scalar_mul(self, g2_aff: bytes, s: bytes) -> bytes:
        """s * Q for a 128-byte affine G2 point (host arithmetic)"""
        _need(g2_aff, 128, "g2_aff")
        _need(s, 32, "s")
        return g2_scalar_mul(g2_aff, s)

    def g2_batch_compress(self, aff: bytes) -> bytes:
        """128-byte affine G2 points -> the 64-byte form ParamsKZG::write stores (inverse of g2_batch_decompress)"""
        return g2_batch_compress(aff)

    def g1_msm_preloaded(self, handle: int, scalars: bytes) -> bytes:
        _need(scalars, 32 * (len(scalars) // 32), "scalars")
        out = C.create_string_buffer(96)
        self._check(self._lib.h2agg_g1_msm_preloaded(self._ctx, handle, scalars, len(scalars) // 32, out))
        return out.raw

    def instance_commitment(self, g_lagrange_handle: int, instance: bytes, max_len: int) -> bytes:
        _need(instance, 32 * (len(instance) // 32), "instance")
        out = C.create_string_buffer(96)
        self._check(self._lib.h2agg_instance_commitment(self._ctx, g_lagrange_handle, instance, len(instance) // 32,
                                                        max_len, out))
        return out.raw

    def g1_msm_device(self, handle: int, d_scalars_ptr: int, n: int) -> bytes:
        out = C.create_string_buffer(96)
        self._check(self._lib.h2agg_g1_msm_device(self._ctx, handle, d_scalars_ptr, n, out))
        return out.raw

    def g1_msm_device_async(self, handle: int, d_scalars_ptr: int, n: int, d_out_ptr: int):
        self._check(self._lib.h2agg_g1_msm_device_async(self._ctx, handle, d_scalars_ptr, n, d_out_ptr))

    # ------------------------------------------------------------------ transcript side
    def poseidon_squeeze_batch(self, elems: bytes, nproofs: int, upto: Sequence[int]) -> bytes:
        """nproofs sponges (T=9, RATE=8, R_F=8, R_P=63): elems [nproofs][nelem] canonical Fr -> [nproofs][len(upto)] challenges"""
        nelem = (len(elems) // 32) // max(nproofs, 1)
        _need(elems, 32 * nelem * nproofs, "elems")
        nsq = len(upto)
        arr = (C.c_uint32 * max(nsq, 1))(*upto)
        out = C.create_string_buffer(max(32 * nproofs * nsq, 1))
        self._check(self._lib.h2agg_poseidon_squeeze_batch(self._ctx, elems, nproofs, nelem, arr, nsq, out))
        return out.raw[:32 * nproofs * nsq]

    def verify_plan_stats(self):
        """(hits, misses, plans kept) of the context's recorded-aggregation cache (h2agg_verify_plan_stats)"""
        h, m, k = C.c_uint64(), C.c_uint64(), C.c_uint64()
        self._check(self._lib.h2agg_verify_plan_stats(self._ctx, C.byref(h), C.byref(m), C.byref(k)))
        return h.value, m.value, k.value

    def last_phases(self) -> str:
        """wall-clock split of the last verify_aggregation call, or the combine / divide / commit split of the last
        kzg_multiopen call (after debug_configure("phases", 1)): h2agg_last_phases"""
        return (self._lib.h2agg_last_phases(self._ctx) or b"").decode()

    def transcript_configure(self, backend: str = "auto"):
        """which backend runs the transcripts' hash chains (Poseidon sponges, SHA-256 / Keccak-256) of this context: "auto" (by
        batch size), "device", "host" (worker threads)"""
        self._check(self._lib.h2agg_transcript_configure(self._ctx, {"auto": 0, "device": 1, "host": 2}[backend]))

    def transcript_read_batch(self, proofs: Sequence[bytes], script: str, consts: bytes = b"", ext_points_aff: bytes = b""):
        """PoseidonTranscriptRead over same-layout proofs -> (points [proof] bytes, challenges [proof] bytes)"""
        nproofs = len(proofs)
        plen = 32 * (script.count("P") + script.count("S"))
        for p in proofs:
            _need(p, plen, "proof")
        npts, nsq, nx = script.count("P"), script.count("Q"), script.count("X")
        _need(consts, 32 * script.count("C"), "consts")
        _need(ext_points_aff, 64 * nx * nproofs, "ext_points_aff")
        pts = C.create_string_buffer(max(64 * npts * nproofs, 1))
        ch = C.create_string_buffer(max(32 * nsq * nproofs, 1))
        sb = script.encode()
        self._check(self._lib.h2agg_transcript_read_batch(self._ctx, b"".join(proofs), plen, nproofs, sb, len(sb), consts,
                                                          len(consts) // 32, ext_points_aff, nx, pts, ch))
        return ([pts.raw[64 * npts * i:64 * npts * (i + 1)] for i in range(nproofs)],
                [ch.raw[32 * nsq * i:32 * nsq * (i + 1)] for i in range(nproofs)])

    def hash_transcript_read_batch(self, kind: str, proofs: Sequence[bytes], script: str, consts: bytes = b"",
                                   ext_points_aff: bytes = b""):
        """ShaRead (transcript/sha.rs) over same-layout proofs, kind "sha256" | "keccak256": points are 64 uncompressed
        bytes -> (points [proof] bytes, challenges [proof] bytes)"""
        args, pts, ch, npts, nsq = _hash_transcript_args(kind, proofs, script, consts, ext_points_aff)
        self._check(self._lib.h2agg_hash_transcript_read_batch(self._ctx, *args, pts, ch))
        nproofs = len(proofs)
        return ([pts.raw[64 * npts * i:64 * npts * (i + 1)] for i in range(nproofs)],
                [ch.raw[32 * nsq * i:32 * nsq * (i + 1)] for i in range(nproofs)])

    # ------------------------------------------------------------------ multi-GPU exchange (RCCL inside the C ABI)
    @staticmethod
    def comm_unique_id() -> bytes:
        """rank 0: the 128-byte RCCL id every rank passes to comm_init_rank"""
        out = C.create_string_buffer(128)
        rc = load_library().h2agg_comm_unique_id(out)
        if rc != OK:
            why = load_library().h2agg_comm_last_error() or b""
            raise H2AggError(rc, "h2agg_comm_unique_id failed: " + (why.decode(errors="replace") or "RCCL error"))
        return out.raw

    def comm_init_rank(self, unique_id: bytes, rank: int, nranks: int):
        _need(unique_id, 128, "unique_id")
        self._check(self._lib.h2agg_comm_init_rank(self._ctx, unique_id, rank, nranks))

    def comm_size(self) -> int:
        """ranks of this context's communicator (0 = none)"""
        return self._lib.h2agg_comm_size(self._ctx)

    def comm_rank(self) -> int:
        """this context's rank in its communicator (-1 = none)"""
        return self._lib.h2agg_comm_rank(self._ctx)

    def allgather_add_points(self, partial_jac: bytes) -> bytes:
        """this rank's partial accumulators (96 B each) -> affine sums over all ranks (64 B each), same on every rank:
        the one collective of the sharded aggregation (all-gather over RCCL + local EC adds)"""
        npts = len(partial_jac) // 96
        _need(partial_jac, 96 * npts, "partial_jac")
        out = C.create_string_buffer(max(64 * npts, 1))
        arr = (C.c_void_p * 1)(self._ctx)
        self._check(self._lib.h2agg_allgather_add_points(arr, 1, partial_jac, npts, out))
        return out.raw[:64 * npts]

    # ------------------------------------------------------------------ pairing (host)
    def pairing_check(self, g1_aff: bytes, g2_aff: bytes) -> bool:
        """prod e(g1_i, g2_i) == 1  (verify.rs:733-739 / EIP-197); G2 = x.c0 || x.c1 || y.c0 || y.c1"""
        n = len(g1_aff) // 64
        _need(g1_aff, 64 * n, "g1_aff")
        _need(g2_aff, 128 * n, "g2_aff")
        ok = C.c_int()
        self._check(self._lib.h2agg_pairing_check(self._ctx, g1_aff, g2_aff, n, C.byref(ok)))
        return bool(ok.value)

    def pairing_product(self, g1_aff: bytes, g2_aff: bytes) -> bytes:
        n = len(g1_aff) // 64
        _need(g1_aff, 64 * n, "g1_aff")
        _need(g2_aff, 128 * n, "g2_aff")
        out = C.create_string_buffer(384)
        self._check(self._lib.h2agg_pairing_product(self._ctx, g1_aff, g2_aff, n, out))
        return out.raw

    def g2_batch_decompress(self, data: bytes) -> bytes:
        """64-byte compressed G2 points (ParamsKZG::write's g2 / s_g2) -> 128-byte affine"""
        n = len(data) // 64
        _need(data, 64 * n, "data")
        out = C.create_string_buffer(max(128 * n, 1))
        self._check(self._lib.h2agg_g2_batch_decompress(self._ctx, data, n, out))
        return out.raw[:128 * n]

    def final_pair_check(self, left_aff: bytes, right_aff: bytes, s_g2: bytes, g2: bytes) -> bool:
        """e(left, [s]_2) * e(right, -[1]_2) == 1"""
        _need(left_aff, 64, "left_aff")
        _need(right_aff, 64, "right_aff")
        _need(s_g2, 128, "s_g2")
        _need(g2, 128, "g2")
        ok = C.c_int()
        self._check(self._lib.h2agg_final_pair_check(self._ctx, left_aff, right_aff, s_g2, g2, C.byref(ok)))
        return bool(ok.value)

    # ------------------------------------------------------------------ tuning / measurement
    def g1_msm_device_batch_async(self, handle: int, d_scalars_ptr: int, n: int, batch: int, d_out_ptr: int):
        self._check(self._lib.h2agg_g1_msm_device_batch_async(self._ctx, handle, C.c_void_p(d_scalars_ptr), n, batch,
                                                              C.c_void_p(d_out_ptr)))

    def msm_configure(self, window_bits: int = 0, reduce_segment: int = 0, big_bucket_threshold: int = 0):
        self._check(self._lib.h2agg_msm_configure(self._ctx, window_bits, reduce_segment, big_bucket_threshold))

    def msm_configure_glv(self, mode: int = 0):
        self._check(self._lib.h2agg_msm_configure_glv(self._ctx, mode))

    def msm_configure_lanes_per_bucket(self, lanes: int = 0):
        self._check(self._lib.h2agg_msm_configure_lanes_per_bucket(self._ctx, lanes))

    def msm_configure_sort(self, sub_bits: int = 0, tile: int = 0):
        self._check(self._lib.h2agg_msm_configure_sort(self._ctx, sub_bits, tile))

    def debug_configure(self, key: str, value: int):
        """h2agg_debug_configure: per-context test hooks (include/h2agg.h "Environment")"""
        self._check(self._lib.h2agg_debug_configure(self._ctx, key.encode(), int(value)))

    def table_may_hold_identity(self, handle: int) -> bool:
        """False when the call that wrote the table stored no identity base (the bucket accumulation then skips the test)"""
        v = C.c_int32(-1)
        self._check(self._lib.h2agg_debug_table_identity(self._ctx, handle, C.byref(v), None))
        return bool(v.value)

    def last_lean_variant(self) -> int:
        """the per-entry decisions the last bucket accumulation kept: 1 = identity test, 2 = endomorphism select; -1: none yet"""
        v = C.c_int32(-1)
        self._check(self._lib.h2agg_debug_table_identity(self._ctx, 0, None, C.byref(v)))
        return v.value

    def msm_set_tail_overlap(self, level: int = 2):
        """0 = off, 1 = only the Horner kernel on a tail stream, 2 = bucket reduction + window sums + Horner"""
        self._check(self._lib.h2agg_msm_set_tail_overlap(self._ctx, int(level)))

    def profile_enable(self, on=True, only_stage: Optional[int] = None):
        """only_stage: index into profile_stages() order -> bracket just that stage (cheaper)."""
        mode = (2 + int(only_stage)) if (on and only_stage is not None) else int(bool(on))
        self._check(self._lib.h2agg_profile_enable(self._ctx, mode))

    def profile_reset(self):
        self._check(self._lib.h2agg_profile_reset(self._ctx))

    def profile_stages(self):
        """-> {stage name: (total_ms, launches)}"""
        out = {}
        for i in range(self._lib.h2agg_profile_stage_count(self._ctx)):
            ms, cnt = C.c_double(), C.c_uint64()
            self._check(self._lib.h2agg_profile_stage_get(self._ctx, i, C.byref(ms), C.byref(cnt)))
            out[self._lib.h2agg_profile_stage_name(self._ctx, i).decode()] = (ms.value, cnt.value)
        return out


def host_sponge_kind() -> str:
    """arithmetic the host sponge runs on here: "ifma" (AVX-512 IFMA) or "scalar" (portable 4 x 64-bit)"""
    return "ifma" if load_library().h2agg_host_sponge_kind() == 1 else "scalar"


def poseidon_squeeze_batch_host(elems: bytes, nproofs: int, upto: Sequence[int], max_threads: int = 0,
                                kernel: Optional[str] = None) -> bytes:
    """the host backend of H2Agg.poseidon_squeeze_batch on its own (h2agg_poseidon_squeeze_batch_host: no context, no device);
    kernel: None = the process-wide choice, "scalar" / "ifma" = force one for this call (ifma only where the CPU has it)"""
    lib = load_library()
    max_threads = (max_threads & 0xffff) | {None: 0, "scalar": 0x10000, "ifma": 0x20000}[kernel]
    nelem = (len(elems) // 32) // max(nproofs, 1)
    _need(elems, 32 * nelem * nproofs, "elems")
    nsq = len(upto)
    arr = (C.c_uint32 * max(nsq, 1))(*upto)
    out = C.create_string_buffer(32 * max(nproofs * nsq, 1))
    rc = lib.h2agg_poseidon_squeeze_batch_host(elems, nproofs, nelem, arr, nsq, out, max_threads)
    if rc != OK:
        raise H2AggError(rc, "h2agg_poseidon_squeeze_batch_host: " + ("element >= r" if rc == ERR_NONCANONICAL else "invalid arguments"))
    return out.raw[:32 * nproofs * nsq]


TRANSCRIPT_KINDS = {"poseidon": 0, "sha256": 1, "keccak256": 2}


def _hash_transcript_args(kind, proofs, script, consts, ext_points_aff):
    nproofs = len(proofs)
    plen = 64 * script.count("P") + 32 * script.count("S")
    for p in proofs:
        _need(p, plen, "proof")
    npts, nsq, nx = script.count("P"), script.count("Q"), script.count("X")
    _need(consts, 32 * script.count("C"), "consts")
    _need(ext_points_aff, 64 * nx * nproofs, "ext_points_aff")
    pts = C.create_string_buffer(max(64 * npts * nproofs, 1))
    ch = C.create_string_buffer(max(32 * nsq * nproofs, 1))
    sb = script.encode()
    k = TRANSCRIPT_KINDS.get(kind, kind)
    return (k, b"".join(proofs), plen, nproofs, sb, len(sb), consts, len(consts) // 32, ext_points_aff, nx), pts, ch, npts, nsq


def hash_transcript_read_batch_host(kind: str, proofs: Sequence[bytes], script: str, consts: bytes = b"",
                                    ext_points_aff: bytes = b"", max_threads: int = 0):
    """the host backend of H2Agg.hash_transcript_read_batch on its own (no context, no device)"""
    args, pts, ch, npts, nsq = _hash_transcript_args(kind, proofs, script, consts, ext_points_aff)
    rc = load_library().h2agg_hash_transcript_read_batch_host(*args, pts, ch, max_threads)
    if rc != OK:
        what = {ERR_BAD_POINT: "invalid point encoding in proof", ERR_NONCANONICAL: "invalid field element encoding in proof"}
        raise (BadPoint if rc == ERR_BAD_POINT else H2AggError)(rc, "h2agg_hash_transcript_read_batch_host: " + what.get(rc, "invalid arguments"))
    nproofs = len(proofs)
    return ([pts.raw[64 * npts * i:64 * npts * (i + 1)] for i in range(nproofs)],
            [ch.raw[32 * nsq * i:32 * nsq * (i + 1)] for i in range(nproofs)])


def hash_digest_host(kind: str, msg: bytes) -> bytes:
    """SHA-256 / Keccak-256 of `msg` by the library's own host digests (h2agg_hash_digest_host)"""
    out = C.create_string_buffer(32)
    rc = load_library().h2agg_hash_digest_host(TRANSCRIPT_KINDS.get(kind, kind), msg, len(msg), out)
    if rc != OK:
        raise H2AggError(rc, "h2agg_hash_digest_host: invalid arguments")
    return out.raw


def host_threads() -> int:
    """worker threads the library may use for per-proof host work (h2agg_host_threads)"""
    return load_library().h2agg_host_threads()


class H2AggGroup:
    """One process driving several GPUs: h2agg_comm_create = a context per device + ncclCommInitAll."""

    def __init__(self, devices: Sequence[int]):
        lib = load_library()
        n = len(devices)
        devs = (C.c_int * n)(*devices)
        ctxs = (C.c_void_p * n)()
        rc = lib.h2agg_comm_create(devs, n, ctxs)
        if rc != OK:
            msg = (lib.h2agg_last_error(ctxs[0]) or b"").decode() if ctxs[0] else "RCCL or a device is not available"
            for cx in ctxs:
                if cx:
                    lib.h2agg_destroy(cx)
            raise H2AggError(rc, "h2agg_comm_create: " + msg)
        self._lib, self._ctxs = lib, ctxs
        self.engines = []
        for i, d in enumerate(devices):          # wrap the contexts so the whole H2Agg surface is usable per device
            e = H2Agg.__new__(H2Agg)
            e._lib, e._ctx, e.device = lib, C.c_void_p(ctxs[i]), d
            self.engines.append(e)

    def allgather_add_points(self, partials: Sequence[bytes]) -> bytes:
        """partials[rank] = that rank's npts Jacobian points -> npts affine sums"""
        n = len(self.engines)
        if len(partials) != n:
            raise ValueError("one partial buffer per device")
        npts = len(partials[0]) // 96
        for p in partials:
            _need(p, 96 * npts, "partial")
        out = C.create_string_buffer(max(64 * npts, 1))
        self.engines[0]._check(self._lib.h2agg_allgather_add_points(self._ctxs, n, b"".join(partials), npts, out))
        return out.raw[:64 * npts]

    def close(self):
        for e in self.engines:
            e.close()
        self.engines = []


# ---------------------------------------------------------------------------------------------------
# EvaluationQuerySchema mirror (halo2-snark-aggregator-api/src/systems/halo2/evaluation.rs).  The AST lives
# in the C++ host layer of libh2agg.so; these classes only hold node ids, so tests read like the
# reference's: `commit(cq) + evalq(cq)`, `scalar(v) * acc + q`, `proof.w_x.eval(...)`.
class CommitQuery:                       # evaluation.rs:7-12
    def __init__(self, key: str, commitment: Optional[bytes] = None, eval: Optional[bytes] = None):
        self.key, self.commitment, self.eval = key, commitment, eval


class SchemaBuilder:
    """Arena of schema nodes bound to one H2Agg context."""

    def __init__(self, eng: H2Agg):
        self.eng = eng
        self._lib = eng._lib
        self._s = C.c_void_p()
        eng._check(self._lib.h2agg_schema_create(eng._ctx, C.byref(self._s)))
        eng._register_builder(self)

    def close(self):
        if getattr(self, "_s", None) and getattr(self.eng, "_ctx", None):
            self._lib.h2agg_schema_destroy(self._s)
        self._s = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _node(self, fn, *args) -> "EvaluationQuerySchema":
        out = C.c_uint32()
        self.eng._check(fn(self._s, *args, C.byref(out)))
        return EvaluationQuerySchema(self, out.value)

    def commit(self, cq: CommitQuery) -> "EvaluationQuerySchema":        # commit!  evaluation.rs:41-46
        _need(cq.commitment, 64, "commitment")
        return self._node(self._lib.h2agg_schema_node_commitment, cq.key.encode(), cq.commitment)

    def evalq(self, cq: CommitQuery) -> "EvaluationQuerySchema":         # eval!    evaluation.rs:48-53
        _need(cq.eval, 32, "eval")
        return self._node(self._lib.h2agg_schema_node_eval, cq.eval)

    def scalar(self, s: bytes) -> "EvaluationQuerySchema":               # scalar!  evaluation.rs:55-60
        _need(s, 32, "scalar")
        return self._node(self._lib.h2agg_schema_node_scalar, s)

    @staticmethod
    def keys_array(keys: Sequence[str]):
        """the query keys as a C string array, built once and reusable across calls (the reference formats its keys once per
        proof too; re-encoding hundreds of Python strings per call costs more than the device work)"""
        return (C.c_char_p * len(keys))(*[k.encode() for k in keys])

    def evaluation_queries(self, keys, commitments: bytes, evals: bytes, wrap: bool = True):
        """n x EvaluationQuery::new in one call -> list of schema nodes ([C_i] + eval_i).  `keys`: strings, or the array
        from keys_array().  wrap=False returns the raw node-id array (accepted by batch_multi_open): a proof has hundreds
        of queries and one Python object per query costs more than the device work."""
        n = len(keys)
        _need(commitments, 64 * n, "commitments")
        _need(evals, 32 * n, "evals")
        arr = keys if isinstance(keys, C.Array) else self.keys_array(keys)
        out = (C.c_uint32 * n)()
        self.eng._check(self._lib.h2agg_schema_evaluation_queries(self._s, n, arr, commitments, evals, out))
        if not wrap:
            return out
        return [EvaluationQuerySchema(self, out[i]) for i in range(n)]

    def query_set_commitment(self, query_node, point_aff: bytes):
        node = query_node.node if isinstance(query_node, EvaluationQuerySchema) else int(query_node)
        _need(point_aff, 64, "point_aff")
        self.eng._check(self._lib.h2agg_schema_query_set_commitment(self._s, node, point_aff))

    def batch_multi_open(self, key: str, rotations: Sequence[int], points: bytes, query_nodes, w: bytes,
                         v: bytes, u: bytes):
        """multiopen.rs:23-102 in the C++ host layer -> (w_x, w_g) schema nodes."""
        nq = len(rotations)
        _need(points, 32 * nq, "points")
        _need(w, 64 * (len(w) // 64), "w")
        _need(v, 32, "v")
        _need(u, 32, "u")
        if len(query_nodes) != nq:
            raise ValueError("one query node per rotation")
        rot = rotations if isinstance(rotations, C.Array) else (C.c_int32 * nq)(*rotations)
        if isinstance(query_nodes, C.Array):
            qn = query_nodes
        else:
            qn = (C.c_uint32 * nq)(*[q.node if isinstance(q, EvaluationQuerySchema) else int(q) for q in query_nodes])
        wx, wg = C.c_uint32(), C.c_uint32()
        self.eng._check(self._lib.h2agg_schema_batch_multi_open(self._s, key.encode(), nq, rot, points, qn,
                                                                len(w) // 64, w, v, u, C.byref(wx), C.byref(wg)))
        return EvaluationQuerySchema(self, wx.value), EvaluationQuerySchema(self, wg.value)

    def shplonk_multi_open(self, key: str, poly_ids: Sequence[int], rotations: Sequence[int], points: bytes, query_nodes,
                           h1: bytes, h2: bytes, y: bytes, v: bytes, u: bytes):
        """the Shplonk verifier of include/h2agg.h (h2agg_schema_shplonk_multi_open) in the C++ host layer -> (left, right)
        schema nodes for evaluate_multiopen_proof: left = commit(H2), right = F + u H2."""
        nq = len(rotations)
        _need(points, 32 * nq, "points")
        _need(h1, 64, "h1")
        _need(h2, 64, "h2")
        _need(y, 32, "y")
        _need(v, 32, "v")
        _need(u, 32, "u")
        if len(query_nodes) != nq or len(poly_ids) != nq:
            raise ValueError("one polynomial id and one query node per rotation")
        ids = poly_ids if isinstance(poly_ids, C.Array) else (C.c_uint32 * max(nq, 1))(*poly_ids)
        rot = rotations if isinstance(rotations, C.Array) else (C.c_int32 * max(nq, 1))(*rotations)
        if isinstance(query_nodes, C.Array):
            qn = query_nodes
        else:
            qn = (C.c_uint32 * max(nq, 1))(*[q.node if isinstance(q, EvaluationQuerySchema) else int(q) for q in query_nodes])
        left, right = C.c_uint32(), C.c_uint32()
        self.eng._check(self._lib.h2agg_schema_shplonk_multi_open(self._s, key.encode(), nq, ids, rot, points, qn, h1, h2, y, v, u,
                                                                  C.byref(left), C.byref(right)))
        return EvaluationQuerySchema(self, left.value), EvaluationQuerySchema(self, right.value)

    def evaluate_multiopen_proof(self, w_x: "EvaluationQuerySchema", w_g: "EvaluationQuerySchema"):
        """verify.rs:705-731 -> (left_aff, right_aff, names)"""
        left, right = C.create_string_buffer(64), C.create_string_buffer(64)
        self.eng._check(self._lib.h2agg_evaluate_multiopen_proof(self._s, w_x.node, w_g.node, left, right))
        return left.raw, right.raw, self.names()

    def evaluate_multiopen_prepare(self, w_x: "EvaluationQuerySchema", w_g: "EvaluationQuerySchema"):
        """the host half of evaluate_multiopen_proof(w_x, w_g) ahead of time (no device work): commitments may still be
        replaced (query_set_commitment) before the evaluation itself"""
        self.eng._check(self._lib.h2agg_evaluate_multiopen_prepare(self._s, w_x.node, w_g.node))

    def names(self):
        need = self._lib.h2agg_schema_names_joined(self._s, None, 0)
        if need == 0:
            return []
        buf = C.create_string_buffer(need)
        self._lib.h2agg_schema_names_joined(self._s, buf, need)
        return buf.raw[:need].decode().split("\n")[:-1]

    def point_list_len(self) -> int:
        return self._lib.h2agg_schema_point_list_len(self._s)


class EvaluationQuerySchema:
    def __init__(self, builder: SchemaBuilder, node: int):
        self.b, self.node = builder, node

    def __add__(self, other):                                            # impl Add  evaluation.rs:62-72
        return self.b._node(self.b._lib.h2agg_schema_node_add, self.node, other.node)

    def __mul__(self, other):                                            # impl Mul  evaluation.rs:74-84
        return self.b._node(self.b._lib.h2agg_schema_node_mul, self.node, other.node)

    def estimate(self) -> int:                                           # evaluation.rs:295-330
        out = C.c_size_t()
        self.b.eng._check(self.b._lib.h2agg_schema_estimate(self.b._s, self.node, C.byref(out)))
        return out.value

    def eval(self):
        """evaluation.rs:172-203 -> (point_jac, scalar or None, names)"""
        jac, sc, has = C.create_string_buffer(96), C.create_string_buffer(32), C.c_int()
        self.b.eng._check(self.b._lib.h2agg_schema_eval(self.b._s, self.node, jac, C.byref(has), sc))
        return jac.raw, (sc.raw if has.value else None), self.b.names()
