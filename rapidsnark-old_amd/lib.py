"""ctypes binding of include/zkhip.h.  Fails loudly when libzkhip.so is absent — there is
no Python or CPU fallback for any compute entry point."""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None


class ZkHipError(RuntimeError):
    pass


def library_path():
    # ZKHIP_LIB: another build of the same library (A/B measurements on one box); never a fallback
    return os.environ.get("ZKHIP_LIB") or os.path.join(_HERE, "libzkhip.so")


class zk_zkey_view(C.Structure):
    _fields_ = [("nVars", C.c_uint32), ("nPublic", C.c_uint32), ("domainSize", C.c_uint32), ("nCoefs", C.c_uint64),
                ("vk_alpha1", C.c_void_p), ("vk_beta1", C.c_void_p), ("vk_beta2", C.c_void_p),
                ("vk_delta1", C.c_void_p), ("vk_delta2", C.c_void_p), ("coefs", C.c_void_p),
                ("pointsA", C.c_void_p), ("pointsB1", C.c_void_p), ("pointsB2", C.c_void_p),
                ("pointsC", C.c_void_p), ("pointsH", C.c_void_p),
                ("coefs_bytes", C.c_uint64), ("pointsA_bytes", C.c_uint64), ("pointsB1_bytes", C.c_uint64),
                ("pointsB2_bytes", C.c_uint64), ("pointsC_bytes", C.c_uint64), ("pointsH_bytes", C.c_uint64)]


class zk_opts(C.Structure):
    _fields_ = [("device", C.c_int32), ("shard_index", C.c_uint32), ("shard_count", C.c_uint32),
                ("window_bits", C.c_uint32), ("flags", C.c_uint32), ("batch", C.c_uint32)]


class zk_proof(C.Structure):
    _fields_ = [("A", C.c_uint8 * 64), ("B", C.c_uint8 * 128), ("C", C.c_uint8 * 64)]


class zk_msm_sums(C.Structure):
    _fields_ = [("pih", C.c_uint8 * 64), ("pi_a", C.c_uint8 * 64), ("pib1", C.c_uint8 * 64),
                ("pi_b", C.c_uint8 * 128), ("pi_c", C.c_uint8 * 64)]


class zk_prover_plan(C.Structure):
    _fields_ = [("size", C.c_uint32), ("window_bits_h", C.c_uint32), ("windows_h", C.c_uint32), ("window_bits_w", C.c_uint32),
                ("windows_w", C.c_uint32), ("precomputed_tables", C.c_uint32), ("msm_a_b1_c_one_launch", C.c_uint32), ("lanes", C.c_uint32),
                ("follow_up_streams", C.c_uint32), ("max_in_flight", C.c_uint32), ("depth_host_witness", C.c_uint32),
                ("depth_resident_witness", C.c_uint32), ("batch", C.c_uint32), ("shard_index", C.c_uint32), ("shard_count", C.c_uint32),
                ("chain_partitioned", C.c_uint32), ("device_bytes_in_use", C.c_uint64), ("device_bytes_total", C.c_uint64),
                ("kernel_launches_last_proof", C.c_uint64), ("table_rows_h", C.c_uint32), ("table_rows_w", C.c_uint32),
                ("bucket_sets_h", C.c_uint32), ("bucket_sets_w", C.c_uint32),
                ("spmv_row_cut", C.c_uint32), ("spmv_long_rows", C.c_uint32), ("spmv_longest_row", C.c_uint32), ("spmv_chunks", C.c_uint32)]


class zk_r1cs_view(C.Structure):
    _fields_ = [("nWires", C.c_uint32), ("nPubOut", C.c_uint32), ("nPubIn", C.c_uint32), ("nPrvIn", C.c_uint32),
                ("nConstraints", C.c_uint32), ("constraints", C.c_void_p), ("constraints_bytes", C.c_uint64)]


class zk_r1cs_report(C.Structure):
    _fields_ = [("size", C.c_uint32), ("failed", C.c_uint64), ("first_failed", C.c_uint32), ("a", C.c_uint8 * 32),
                ("b", C.c_uint8 * 32), ("c", C.c_uint8 * 32), ("one_ok", C.c_uint32), ("first_unreduced", C.c_uint32)]


class zk_ptau_view(C.Structure):
    _fields_ = [("power", C.c_uint32), ("alpha1", C.c_void_p), ("beta1", C.c_void_p), ("beta2", C.c_void_p),
                ("lagrange_g1", C.c_void_p), ("lagrange_g2", C.c_void_p), ("lagrange_alpha_g1", C.c_void_p), ("lagrange_beta_g1", C.c_void_p),
                ("lagrange_g1_bytes", C.c_uint64), ("lagrange_g2_bytes", C.c_uint64), ("lagrange_alpha_g1_bytes", C.c_uint64),
                ("lagrange_beta_g1_bytes", C.c_uint64)]


class zk_setup_sizes(C.Structure):
    _fields_ = [("nVars", C.c_uint32), ("nPublic", C.c_uint32), ("domainSize", C.c_uint32), ("log_domain", C.c_uint32), ("nCoefs", C.c_uint64)]


class zk_ptau_powers_view(C.Structure):
    _fields_ = [("power", C.c_uint32), ("tau_g1", C.c_void_p), ("tau_g2", C.c_void_p), ("alpha_tau_g1", C.c_void_p), ("beta_tau_g1", C.c_void_p),
                ("tau_g1_bytes", C.c_uint64), ("tau_g2_bytes", C.c_uint64), ("alpha_tau_g1_bytes", C.c_uint64), ("beta_tau_g1_bytes", C.c_uint64)]


class zk_ptau_lagrange_sizes(C.Structure):
    _fields_ = [("lagrange_g1_bytes", C.c_uint64), ("lagrange_g2_bytes", C.c_uint64), ("lagrange_alpha_g1_bytes", C.c_uint64),
                ("lagrange_beta_g1_bytes", C.c_uint64), ("device_bytes", C.c_uint64)]


class zk_ptau_lagrange_out(C.Structure):
    _fields_ = [("lagrange_g1", C.c_void_p), ("lagrange_g2", C.c_void_p), ("lagrange_alpha_g1", C.c_void_p), ("lagrange_beta_g1", C.c_void_p)]


class zk_zkey_contrib_view(C.Structure):
    _fields_ = [("vk_delta1", C.c_void_p), ("vk_delta2", C.c_void_p), ("pointsC", C.c_void_p), ("pointsH", C.c_void_p),
                ("pointsC_bytes", C.c_uint64), ("pointsH_bytes", C.c_uint64)]


class zk_zkey_contrib_sizes(C.Structure):
    _fields_ = [("pointsC_bytes", C.c_uint64), ("pointsH_bytes", C.c_uint64), ("chunk_points", C.c_uint64), ("device_bytes", C.c_uint64)]


class zk_zkey_contrib_out(C.Structure):
    _fields_ = [("vk_delta1", C.c_void_p), ("vk_delta2", C.c_void_p), ("pointsC", C.c_void_p), ("pointsH", C.c_void_p)]


class zk_vkey_view(C.Structure):
    _fields_ = [("vk_alpha1", C.c_void_p), ("vk_beta2", C.c_void_p), ("vk_gamma2", C.c_void_p), ("vk_delta2", C.c_void_p),
                ("IC", C.c_void_p), ("nPublic", C.c_uint32)]


class zk_vkey_plan(C.Structure):
    _fields_ = [("coop_max", C.c_uint32), ("last_path", C.c_uint32), ("last_launches", C.c_uint32), ("reserved", C.c_uint32),
                ("proofs_coop", C.c_uint64), ("proofs_lanes", C.c_uint64)]


class zk_vkey_batch_report(C.Structure):
    _fields_ = [("size", C.c_uint32), ("group", C.c_uint32), ("groups", C.c_uint64), ("groups_failed", C.c_uint64),
                ("proofs_rechecked", C.c_uint64), ("malformed", C.c_uint64), ("launches", C.c_uint32), ("reserved", C.c_uint32)]


class zk_vkey_set_plan(C.Structure):
    _fields_ = [("size", C.c_uint32), ("n_keys", C.c_uint32), ("last_path", C.c_uint32), ("last_launches", C.c_uint32),
                ("last_waves_padded", C.c_uint64), ("proofs_coop", C.c_uint64), ("proofs_lanes", C.c_uint64)]


class zk_vkey_set_batch_report(C.Structure):
    _fields_ = [("size", C.c_uint32), ("group", C.c_uint32), ("group_keys", C.c_uint32), ("launches", C.c_uint32),
                ("groups", C.c_uint64), ("groups_failed", C.c_uint64), ("segments", C.c_uint64),
                ("proofs_rechecked", C.c_uint64), ("malformed", C.c_uint64)]


class zk_ptau_file_view(C.Structure):
    _fields_ = [("power", C.c_uint32), ("sec", C.c_void_p * 16), ("sec_bytes", C.c_uint64 * 16)]


class zk_ptau_check_sizes_t(C.Structure):
    _fields_ = [("prepared", C.c_uint32), ("chunk_points", C.c_uint64), ("device_bytes", C.c_uint64)]


class zk_ptau_report(C.Structure):
    _fields_ = [("verdict", C.c_uint32), ("failed", C.c_uint32), ("lagrange_failed", C.c_uint32 * 4), ("bad_section", C.c_uint32),
                ("bad_kind", C.c_uint32), ("bad_index", C.c_uint64)]


class zk_ptau_contrib_sizes(C.Structure):
    _fields_ = [("tau_g1_bytes", C.c_uint64), ("tau_g2_bytes", C.c_uint64), ("alpha_tau_g1_bytes", C.c_uint64), ("beta_tau_g1_bytes", C.c_uint64),
                ("beta_g2_bytes", C.c_uint64), ("chunk_points", C.c_uint64), ("device_bytes", C.c_uint64)]


class zk_ptau_contrib_out(C.Structure):
    _fields_ = [("tau_g1", C.c_void_p), ("tau_g2", C.c_void_p), ("alpha_tau_g1", C.c_void_p), ("beta_tau_g1", C.c_void_p), ("beta_g2", C.c_void_p)]


class zk_zkey_verify_view(C.Structure):
    _fields_ = [("key", zk_zkey_view), ("vk_gamma2", C.c_void_p), ("pointsIC", C.c_void_p), ("pointsIC_bytes", C.c_uint64)]


class zk_zkey_verify_sizes_t(C.Structure):
    _fields_ = [("log_domain", C.c_uint32), ("shape_failed", C.c_uint32), ("chunk_points", C.c_uint64), ("device_bytes", C.c_uint64)]


class zk_zkey_verify_report(C.Structure):
    _fields_ = [("size", C.c_uint32), ("verdict", C.c_uint32), ("failed", C.c_uint32), ("not_checked", C.c_uint32), ("shape_failed", C.c_uint32),
                ("bad_section", C.c_uint32), ("bad_kind", C.c_uint32), ("bad_index", C.c_uint64), ("coef_rows_differing", C.c_uint64),
                ("coef_first_row", C.c_uint32), ("delta_is_generator", C.c_uint32)]


class zk_kzg_view(C.Structure):
    _fields_ = [("power", C.c_uint32), ("tau_g1", C.c_void_p), ("tau_g1_bytes", C.c_uint64), ("tau_g2", C.c_void_p), ("tau_g2_bytes", C.c_uint64),
                ("lagrange_g1", C.c_void_p), ("lagrange_g1_bytes", C.c_uint64)]


class zk_kzg_plan(C.Structure):
    _fields_ = [("size", C.c_uint32), ("lagrange_log_n", C.c_uint32), ("max_coeffs", C.c_uint64), ("device_bytes", C.c_uint64),
                ("seg", C.c_uint32), ("last_launches", C.c_uint32)]


class zk_plonk_circuit_view(C.Structure):
    _fields_ = [("log_n", C.c_uint32), ("basis", C.c_uint32)] + [(name, C.c_void_p) for name in ("ql", "qr", "qm", "qo", "qc", "s1", "s2", "s3")] + \
               [("k1", C.c_uint8 * 32), ("k2", C.c_uint8 * 32), ("shift", C.c_void_p)]


class zk_plonk_circuit_plan(C.Structure):
    _fields_ = [("size", C.c_uint32), ("log_n", C.c_uint32), ("points", C.c_uint64), ("device_bytes", C.c_uint64), ("seg", C.c_uint32),
                ("last_launches", C.c_uint32)]


class zk_plonk_opening_plan(C.Structure):
    _fields_ = [("size", C.c_uint32), ("log_n", C.c_uint32), ("device_bytes", C.c_uint64), ("seg", C.c_uint32), ("last_launches", C.c_uint32),
                ("pending", C.c_uint32), ("reserved", C.c_uint32)]


class zk_plonk_vkey(C.Structure):
    _fields_ = [("size", C.c_uint32), ("log_n", C.c_uint32), ("n_public", C.c_uint64), ("k1", C.c_uint8 * 32), ("k2", C.c_uint8 * 32)] + \
               [(name, C.c_uint8 * 64) for name in ("qm", "ql", "qr", "qo", "qc", "s1", "s2", "s3")] + [("tau_g2", C.c_uint8 * 128)]


class zk_plonk_prover_plan(C.Structure):
    _fields_ = [("size", C.c_uint32), ("log_n", C.c_uint32), ("n_witness", C.c_uint64), ("n_public", C.c_uint64), ("device_bytes", C.c_uint64),
                ("scan_seg", C.c_uint32), ("quot_seg", C.c_uint32), ("open_seg", C.c_uint32), ("kzg_seg", C.c_uint32), ("last_launches", C.c_uint32),
                ("round_launches", C.c_uint32 * 5)]


class zk_plonk_prover_many_plan(C.Structure):
    _fields_ = [("size", C.c_uint32), ("batch", C.c_uint32), ("table_batch", C.c_uint32), ("window_bits", C.c_uint32), ("table_rows", C.c_uint32),
                ("reserved", C.c_uint32), ("table_bytes", C.c_uint64), ("slot_bytes", C.c_uint64), ("msm_bytes", C.c_uint64),
                ("last_chunks", C.c_uint32), ("last_multiplications", C.c_uint32), ("last_launches", C.c_uint32), ("last_drains", C.c_uint32),
                ("last_refused", C.c_uint32), ("reserved2", C.c_uint32)]


class zk_plonk_verifier_plan(C.Structure):
    _fields_ = [("size", C.c_uint32), ("log_n", C.c_uint32), ("n_public", C.c_uint64), ("device_bytes", C.c_uint64), ("chunk", C.c_uint64),
                ("last_launches", C.c_uint32), ("last_chunks", C.c_uint32)]


class zk_plonk_batch_report(C.Structure):
    _fields_ = [("size", C.c_uint32), ("group", C.c_uint32), ("groups", C.c_uint64), ("groups_failed", C.c_uint64), ("proofs_rechecked", C.c_uint64),
                ("malformed", C.c_uint64), ("launches", C.c_uint32), ("chunks", C.c_uint32)]


class zk_plonk_verifier_set_plan(C.Structure):
    _fields_ = [("size", C.c_uint32), ("n_keys", C.c_uint32), ("max_n_public", C.c_uint64), ("device_bytes", C.c_uint64), ("chunk", C.c_uint64),
                ("last_launches", C.c_uint32), ("last_chunks", C.c_uint32)]


class zk_plonk_set_batch_report(C.Structure):
    _fields_ = [("size", C.c_uint32), ("group", C.c_uint32), ("launches", C.c_uint32), ("chunks", C.c_uint32), ("groups", C.c_uint64),
                ("groups_failed", C.c_uint64), ("segments", C.c_uint64), ("proofs_rechecked", C.c_uint64), ("malformed", C.c_uint64)]


class zk_plonk_r1cs_plan(C.Structure):
    _fields_ = [("size", C.c_uint32), ("log_n", C.c_uint32), ("rows", C.c_uint64), ("n_public", C.c_uint64), ("n_wires", C.c_uint64),
                ("n_additions", C.c_uint64), ("n_witness", C.c_uint64), ("terms", C.c_uint64), ("device_bytes", C.c_uint64), ("seg", C.c_uint32),
                ("sort_passes", C.c_uint32), ("last_launches", C.c_uint32), ("reserved", C.c_uint32)]


class zk_setup_out(C.Structure):
    _fields_ = [("coefs", C.c_void_p), ("pointsIC", C.c_void_p), ("pointsA", C.c_void_p), ("pointsB1", C.c_void_p),
                ("pointsB2", C.c_void_p), ("pointsC", C.c_void_p), ("pointsH", C.c_void_p)]


def prover_info(lib, handle):
    """zk_prover_info -> dict: the launch plan zk_prover_create chose (window bits, A|B1|C in one launch, lanes, depths,
    the long-row cut of A.w / B.w and what it found: spmv_row_cut, spmv_long_rows, spmv_longest_row, spmv_chunks)."""
    plan = zk_prover_plan()
    plan.size = C.sizeof(zk_prover_plan)
    check(lib.zk_prover_info(handle, C.byref(plan)))
    return {name: int(getattr(plan, name)) for name, _ in zk_prover_plan._fields_ if name != "size"}


def multi_prover_shard_info(lib, handle, shard):
    """zk_multi_prover_shard_info -> prover_info's dict for one shard of a zk_multi_prover"""
    plan = zk_prover_plan()
    plan.size = C.sizeof(zk_prover_plan)
    check(lib.zk_multi_prover_shard_info(handle, shard, C.byref(plan)))
    return {name: int(getattr(plan, name)) for name, _ in zk_prover_plan._fields_ if name != "size"}


ZK_FLAG_TIMINGS = 1
ZK_FLAG_PRECOMP = 2
ZK_FLAG_PARTITIONED_CHAIN = 4
ZK_FLAG_SPARSE_WITNESS = 8
ZK_FLAG_PRECOMP_HALF = 16


def precomp_flags(precomp):
    """The `precomp` option of the bindings -> ZK_FLAG_*: False / 0 = tables as in the zkey, True / 1 = a table row per
    window (ZK_FLAG_PRECOMP), 2 = a row per second window (ZK_FLAG_PRECOMP_HALF: 7 instead of 13 x the table memory)."""
    mode = int(precomp)
    if mode not in (0, 1, 2):
        raise ValueError("precomp: 0, 1 or 2")
    return (0, ZK_FLAG_PRECOMP, ZK_FLAG_PRECOMP | ZK_FLAG_PRECOMP_HALF)[mode]
ZK_STEP_CROSS_INVERSE, ZK_STEP_LOCAL, ZK_STEP_CROSS_FORWARD, ZK_STEP_FINISH = 1, 2, 3, 4
ZK_T_NAMES = ["spmv", "ntt_chain_wall", "sort_h", "msm_h_wall", "join_wait", "msm_reduce", "total_device", "g1_l1_kernel", "g2_l1_kernel", "wtns_h2d"]

# every symbol include/zkhip.h declares (tests check the library exports all of them)
EXPORTS = ["zk_last_error", "zk_device_count", "zk_prover_create", "zk_prover_destroy", "zk_prove", "zk_prove_dev",
           "zk_prove_dev_submit", "zk_prove_submit", "zk_prove_batch_submit", "zk_prove_batch_collect", "zk_host_alloc", "zk_host_free", "zk_prove_collect", "zk_prover_reserve", "zk_prover_info", "zk_prove_msm_collect", "zk_prove_msm_dev", "zk_prove_msm", "zk_prove_finish", "zk_prover_timings", "zk_fr_mul_vec",
           "zk_fq_mul_vec", "zk_fr_coef_accumulate", "zk_fr_ntt", "zk_fr_abc_to_h", "zk_msm_g1", "zk_msm_g2", "zk_proof_to_json",
           "zk_public_to_json", "zk_synth_chain_g1", "zk_synth_chain_g2", "zk_fixed_base_g1", "zk_fixed_base_g2", "zk_g1_mul", "zk_g2_mul", "zk_assemble",
           "zk_multi_prover_create", "zk_multi_prover_destroy", "zk_multi_prove", "zk_multi_prove_submit", "zk_multi_prove_collect",
           "zk_multi_prover_info", "zk_multi_prover_shard_info", "zk_shard_info", "zk_shard_set_exchange", "zk_shard_begin", "zk_shard_step",
           "zk_r1cs_create", "zk_r1cs_destroy", "zk_r1cs_check", "zk_r1cs_check_dev", "zk_r1cs_match_zkey",
           "zk_groth16_setup_sizes", "zk_groth16_setup",
           "zk_g1_lagrange", "zk_g2_lagrange", "zk_ptau_prepare_sizes", "zk_ptau_prepare",
           "zk_g1_scale", "zk_g1_scale_plan", "zk_zkey_contribute_sizes", "zk_zkey_contribute",
           "zk_pairing", "zk_vkey_create", "zk_vkey_destroy", "zk_vkey_verify", "zk_vkey_info", "zk_pairing_last_path",
           "zk_vkey_verify_batch", "zk_vkey_set_create", "zk_vkey_set_destroy", "zk_vkey_set_verify", "zk_vkey_set_info", "zk_vkey_set_verify_batch",
           "zk_g2_in_subgroup", "zk_g1_power_msm", "zk_g2_power_msm", "zk_fr_power_dft", "zk_ptau_check_sizes", "zk_ptau_check",
           "zk_zkey_verify_sizes", "zk_zkey_verify",
           "zk_g1_mul_vec", "zk_g2_mul_vec", "zk_g1_power_scale", "zk_g2_power_scale", "zk_glv_split", "zk_ptau_contribute_sizes", "zk_ptau_contribute",
           "zk_fr_poly_divide", "zk_kzg_create", "zk_kzg_destroy", "zk_kzg_info", "zk_kzg_commit", "zk_kzg_open", "zk_kzg_verify", "zk_kzg_verify_batch",
           "zk_fr_batch_inverse", "zk_fr_prefix_product", "zk_fr_grand_product", "zk_plonk_permutation_product", "zk_msm_sort",
           "zk_fr_coset_ntt", "zk_plonk_circuit_create", "zk_plonk_circuit_destroy", "zk_plonk_circuit_info", "zk_plonk_quotient",
           "zk_fr_poly_eval", "zk_plonk_opening_create", "zk_plonk_opening_destroy", "zk_plonk_opening_info", "zk_plonk_evaluate", "zk_plonk_open",
           "zk_keccak256", "zk_plonk_prover_create", "zk_plonk_prover_destroy", "zk_plonk_prover_vkey", "zk_plonk_prover_info", "zk_plonk_prove",
           "zk_plonk_verify",
           "zk_plonk_r1cs_create", "zk_plonk_r1cs_destroy", "zk_plonk_r1cs_info", "zk_plonk_r1cs_circuit", "zk_plonk_r1cs_extend",
           "zk_plonk_prover_create_r1cs", "zk_plonk_prove_r1cs",
           "zk_plonk_prove_many", "zk_plonk_prove_r1cs_many", "zk_plonk_prover_commit_many", "zk_plonk_prover_many_info",
           "zk_plonk_verifier_create", "zk_plonk_verifier_destroy", "zk_plonk_verifier_info", "zk_plonk_verifier_verify", "zk_plonk_verifier_challenges",
           "zk_plonk_verifier_verify_batch", "zk_plonk_verifier_batch_sums",
           "zk_plonk_verifier_set_create", "zk_plonk_verifier_set_destroy", "zk_plonk_verifier_set_info", "zk_plonk_verifier_set_verify",
           "zk_plonk_verifier_set_verify_batch", "zk_plonk_verifier_set_batch_sums"]
ZK_SCAN_EXCLUSIVE = 1
ZK_KZG_MONOMIAL, ZK_KZG_LAGRANGE, ZK_KZG_NO_LAGRANGE = 0, 1, 0xffffffff
ZK_SCALE_PLAN_MAX = 130
ZK_VERIFY_OK, ZK_VERIFY_INVALID, ZK_VERIFY_MALFORMED = 0, 1, 2
ZK_VERIFY_PATH_LANES, ZK_VERIFY_PATH_COOP, ZK_VERIFY_PATH_BATCH = 0, 1, 2
ZK_PTAU_OK, ZK_PTAU_INVALID, ZK_PTAU_MALFORMED = 0, 1, 2


def load_library():
    global _LIB
    if _LIB is not None:
        return _LIB
    path = library_path()
    if not os.path.exists(path):
        raise ZkHipError("libzkhip.so not built (%s): run `python -c 'import __graft_entry__ as g; g.build()'` "
                         "or `make -C rapidsnark-old_amd/csrc`; there is no CPU fallback" % path)
    # six streams per prover: the HIP runtime's default of 4 hardware queues aliases them and the
    # witness upload of proof k+1 then queues behind proof k (csrc/prover_create.hip); read at HIP init
    os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")
    try:
        # torch wheels bundle their own libamdhip64; load it FIRST so this process holds ONE HIP
        # runtime (two runtimes => the second one sees "No HIP GPUs are available").
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = C.CDLL(path)
    lib.zk_last_error.restype = C.c_char_p
    u8p = C.c_void_p
    lib.zk_device_count.argtypes = [C.POINTER(C.c_int)]
    lib.zk_prover_create.argtypes = [C.POINTER(C.c_void_p), C.POINTER(zk_zkey_view), C.POINTER(zk_opts)]
    lib.zk_prover_destroy.argtypes = [C.c_void_p]
    lib.zk_prover_destroy.restype = None
    lib.zk_prove.argtypes = [C.c_void_p, u8p, u8p, u8p, C.POINTER(zk_proof)]
    lib.zk_prove_dev.argtypes = [C.c_void_p, C.c_void_p, u8p, u8p, C.POINTER(zk_proof)]
    lib.zk_prove_dev_submit.argtypes = [C.c_void_p, C.c_void_p, u8p, u8p]
    lib.zk_prove_submit.argtypes = [C.c_void_p, u8p, u8p, u8p]
    lib.zk_prove_batch_submit.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, u8p, u8p]
    lib.zk_prove_batch_collect.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
    lib.zk_host_alloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    lib.zk_host_free.argtypes = [C.c_void_p]
    lib.zk_host_free.restype = None
    lib.zk_prove_collect.argtypes = [C.c_void_p, C.POINTER(zk_proof)]
    lib.zk_prove_msm_collect.argtypes = [C.c_void_p, C.POINTER(zk_msm_sums)]
    lib.zk_prove_msm.argtypes = [C.c_void_p, u8p, C.POINTER(zk_msm_sums)]
    lib.zk_prove_msm_dev.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(zk_msm_sums)]
    lib.zk_prove_finish.argtypes = [C.c_void_p, C.POINTER(zk_msm_sums), C.c_uint32, u8p, u8p, C.POINTER(zk_proof)]
    lib.zk_assemble.argtypes = [u8p, u8p, u8p, u8p, u8p, C.POINTER(zk_msm_sums), C.c_uint32, u8p, u8p, C.POINTER(zk_proof)]
    lib.zk_prover_timings.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.c_uint32]
    if hasattr(lib, "zk_prover_reserve"):      # (ZKHIP_LIB may name an older build of the library: same-box A/B runs)
        lib.zk_prover_reserve.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32]
    if hasattr(lib, "zk_prover_info"):
        lib.zk_prover_info.argtypes = [C.c_void_p, C.POINTER(zk_prover_plan)]
    lib.zk_multi_prover_create.argtypes = [C.POINTER(C.c_void_p), C.POINTER(zk_zkey_view), C.POINTER(C.c_int32), C.c_uint32, C.POINTER(zk_opts)]
    lib.zk_multi_prover_destroy.argtypes = [C.c_void_p]
    lib.zk_multi_prover_destroy.restype = None
    lib.zk_multi_prove.argtypes = [C.c_void_p, u8p, u8p, u8p, C.POINTER(zk_proof)]
    lib.zk_multi_prove_submit.argtypes = [C.c_void_p, u8p, u8p, u8p]
    lib.zk_multi_prove_collect.argtypes = [C.c_void_p, C.POINTER(zk_proof)]
    lib.zk_multi_prover_info.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    lib.zk_multi_prover_shard_info.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(zk_prover_plan)]
    lib.zk_shard_info.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)]
    lib.zk_shard_set_exchange.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    lib.zk_shard_begin.argtypes = [C.c_void_p, u8p, C.c_void_p, u8p, u8p, C.c_void_p]
    lib.zk_shard_step.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    for name in ("zk_fr_mul_vec", "zk_fq_mul_vec"):
        getattr(lib, name).argtypes = [u8p, u8p, u8p, C.c_uint64]
    lib.zk_fr_coef_accumulate.argtypes = [u8p, u8p, u8p, C.c_uint64, C.c_uint32, u8p, C.c_uint32]
    lib.zk_fr_ntt.argtypes = [u8p, C.c_uint64, C.c_int]
    lib.zk_fr_abc_to_h.argtypes = [u8p, u8p, u8p, C.c_uint64]
    lib.zk_msm_g1.argtypes = [u8p, u8p, u8p, C.c_uint64]
    lib.zk_msm_g2.argtypes = [u8p, u8p, u8p, C.c_uint64]
    if hasattr(lib, "zk_msm_sort"):
        lib.zk_msm_sort.argtypes = [u8p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(zk_msm_sort_plan), C.c_void_p, C.c_void_p]
    lib.zk_synth_chain_g1.argtypes = [u8p, C.c_uint64, u8p, u8p]
    lib.zk_synth_chain_g2.argtypes = [u8p, C.c_uint64, u8p, u8p]
    lib.zk_fixed_base_g1.argtypes = [u8p, u8p, u8p, C.c_uint64]
    lib.zk_fixed_base_g2.argtypes = [u8p, u8p, u8p, C.c_uint64]
    lib.zk_g1_mul.argtypes = [u8p, u8p, u8p]
    lib.zk_g2_mul.argtypes = [u8p, u8p, u8p]
    lib.zk_proof_to_json.argtypes = [C.POINTER(zk_proof), C.c_char_p, C.c_size_t]
    lib.zk_proof_to_json.restype = C.c_size_t
    lib.zk_public_to_json.argtypes = [u8p, C.c_uint32, C.c_char_p, C.c_size_t]
    lib.zk_public_to_json.restype = C.c_size_t
    if hasattr(lib, "zk_r1cs_create"):
        lib.zk_r1cs_create.argtypes = [C.POINTER(C.c_void_p), C.POINTER(zk_r1cs_view), C.c_int32]
        lib.zk_r1cs_destroy.argtypes = [C.c_void_p]
        lib.zk_r1cs_destroy.restype = None
        lib.zk_r1cs_check.argtypes = [C.c_void_p, u8p, C.c_uint32, C.POINTER(zk_r1cs_report)]
        lib.zk_r1cs_check_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(zk_r1cs_report)]
        lib.zk_r1cs_match_zkey.argtypes = [C.c_void_p, C.POINTER(zk_zkey_view), C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)]
    if hasattr(lib, "zk_groth16_setup"):
        lib.zk_groth16_setup_sizes.argtypes = [C.POINTER(zk_r1cs_view), C.POINTER(zk_ptau_view), C.POINTER(zk_setup_sizes)]
        lib.zk_groth16_setup.argtypes = [C.POINTER(zk_r1cs_view), C.POINTER(zk_ptau_view), C.c_int32, C.POINTER(zk_setup_out)]
    if hasattr(lib, "zk_ptau_prepare"):
        lib.zk_g1_lagrange.argtypes = [u8p, u8p, C.c_uint64, C.c_uint32, C.c_int32]
        lib.zk_g2_lagrange.argtypes = [u8p, u8p, C.c_uint64, C.c_uint32, C.c_int32]
        lib.zk_ptau_prepare_sizes.argtypes = [C.POINTER(zk_ptau_powers_view), C.POINTER(zk_ptau_lagrange_sizes)]
        lib.zk_ptau_prepare.argtypes = [C.POINTER(zk_ptau_powers_view), C.c_int32, C.POINTER(zk_ptau_lagrange_out)]
    if hasattr(lib, "zk_g1_scale"):
        lib.zk_g1_scale.argtypes = [u8p, u8p, C.c_uint64, u8p, C.c_int32]
        lib.zk_g1_scale_plan.argtypes = [u8p, C.POINTER(C.c_int8), C.POINTER(C.c_int8), C.c_uint32, C.POINTER(C.c_uint32)]
        lib.zk_zkey_contribute_sizes.argtypes = [C.POINTER(zk_zkey_contrib_view), C.POINTER(zk_zkey_contrib_sizes)]
        lib.zk_zkey_contribute.argtypes = [C.POINTER(zk_zkey_contrib_view), u8p, C.c_int32, C.POINTER(zk_zkey_contrib_out)]
    if hasattr(lib, "zk_pairing"):
        lib.zk_pairing.argtypes = [u8p, u8p, u8p, C.c_uint64, C.c_uint32, C.c_int32]
        lib.zk_vkey_create.argtypes = [C.POINTER(C.c_void_p), C.POINTER(zk_vkey_view), C.c_int32]
        lib.zk_vkey_destroy.argtypes = [C.c_void_p]
        lib.zk_vkey_destroy.restype = None
        lib.zk_vkey_verify.argtypes = [C.c_void_p, u8p, u8p, C.c_uint64, u8p]
    if hasattr(lib, "zk_vkey_info"):
        lib.zk_vkey_info.argtypes = [C.c_void_p, C.POINTER(zk_vkey_plan)]
        lib.zk_pairing_last_path.argtypes = []
        lib.zk_pairing_last_path.restype = C.c_int
    if hasattr(lib, "zk_vkey_verify_batch"):
        lib.zk_vkey_verify_batch.argtypes = [C.c_void_p, u8p, u8p, C.c_uint64, u8p, u8p, C.POINTER(zk_vkey_batch_report)]
    if hasattr(lib, "zk_vkey_set_create"):
        lib.zk_vkey_set_create.argtypes = [C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_uint32]
        lib.zk_vkey_set_destroy.argtypes = [C.c_void_p]
        lib.zk_vkey_set_destroy.restype = None
        lib.zk_vkey_set_verify.argtypes = [C.c_void_p, u8p, C.c_void_p, u8p, C.c_uint64, C.c_uint64, u8p]
        lib.zk_vkey_set_info.argtypes = [C.c_void_p, C.POINTER(zk_vkey_set_plan)]
    if hasattr(lib, "zk_vkey_set_verify_batch"):
        lib.zk_vkey_set_verify_batch.argtypes = [C.c_void_p, u8p, C.c_void_p, u8p, C.c_uint64, C.c_uint64, u8p, u8p,
                                                 C.POINTER(zk_vkey_set_batch_report)]
    if hasattr(lib, "zk_ptau_check"):
        lib.zk_g2_in_subgroup.argtypes = [u8p, u8p, C.c_uint64, C.c_int32]
        lib.zk_g1_power_msm.argtypes = [u8p, u8p, C.c_uint64, u8p, C.c_uint64, C.c_int32]
        lib.zk_g2_power_msm.argtypes = [u8p, u8p, C.c_uint64, u8p, C.c_uint64, C.c_int32]
        lib.zk_fr_power_dft.argtypes = [u8p, u8p, C.c_uint32, C.c_int32]
        lib.zk_ptau_check_sizes.argtypes = [C.POINTER(zk_ptau_file_view), C.POINTER(zk_ptau_check_sizes_t)]
        lib.zk_ptau_check.argtypes = [C.POINTER(zk_ptau_file_view), u8p, C.c_int32, C.POINTER(zk_ptau_report)]
    if hasattr(lib, "zk_zkey_verify"):
        lib.zk_zkey_verify_sizes.argtypes = [C.POINTER(zk_r1cs_view), C.POINTER(zk_ptau_view), C.POINTER(zk_zkey_verify_view),
                                             C.POINTER(zk_zkey_verify_sizes_t)]
        lib.zk_zkey_verify.argtypes = [C.POINTER(zk_r1cs_view), C.POINTER(zk_ptau_view), C.POINTER(zk_zkey_verify_view), u8p, C.c_int32,
                                       C.POINTER(zk_zkey_verify_report)]
    if hasattr(lib, "zk_ptau_contribute"):
        lib.zk_g1_mul_vec.argtypes = [u8p, u8p, u8p, C.c_uint64, C.c_int32]
        lib.zk_g2_mul_vec.argtypes = [u8p, u8p, u8p, C.c_uint64, C.c_int32]
        lib.zk_g1_power_scale.argtypes = [u8p, u8p, C.c_uint64, u8p, C.c_uint64, u8p, C.c_int32]
        lib.zk_g2_power_scale.argtypes = [u8p, u8p, C.c_uint64, u8p, C.c_uint64, u8p, C.c_int32]
        lib.zk_glv_split.argtypes = [u8p, u8p, u8p]
        lib.zk_ptau_contribute_sizes.argtypes = [C.POINTER(zk_ptau_file_view), C.POINTER(zk_ptau_contrib_sizes)]
        lib.zk_ptau_contribute.argtypes = [C.POINTER(zk_ptau_file_view), u8p, u8p, u8p, C.c_int32, C.POINTER(zk_ptau_contrib_out)]
    if hasattr(lib, "zk_kzg_create"):
        lib.zk_fr_poly_divide.argtypes = [u8p, u8p, u8p, C.c_uint64, u8p, C.c_int32]
        lib.zk_kzg_create.argtypes = [C.POINTER(C.c_void_p), C.POINTER(zk_kzg_view), C.c_uint64, C.c_uint32, C.c_int32]
        lib.zk_kzg_destroy.argtypes = [C.c_void_p]
        lib.zk_kzg_destroy.restype = None
        lib.zk_kzg_info.argtypes = [C.c_void_p, C.POINTER(zk_kzg_plan)]
        lib.zk_kzg_commit.argtypes = [C.c_void_p, u8p, u8p, C.c_uint64, C.c_uint64, C.c_uint32]
        lib.zk_kzg_open.argtypes = [C.c_void_p, u8p, u8p, u8p, C.c_uint64, C.c_uint64, u8p]
        lib.zk_kzg_verify.argtypes = [C.c_void_p, u8p, u8p, u8p, u8p, C.c_uint64, u8p]
        lib.zk_kzg_verify_batch.argtypes = [C.c_void_p, u8p, u8p, u8p, u8p, C.c_uint64, u8p, u8p]
    if hasattr(lib, "zk_fr_batch_inverse"):
        lib.zk_fr_batch_inverse.argtypes = [u8p, u8p, C.c_uint64, C.POINTER(C.c_uint64), C.c_int32]
        lib.zk_fr_prefix_product.argtypes = [u8p, u8p, C.c_uint64, C.c_uint32, C.c_int32]
        lib.zk_fr_grand_product.argtypes = [u8p, u8p, u8p, u8p, C.c_uint64, C.c_int32]
        lib.zk_plonk_permutation_product.argtypes = [u8p, u8p, u8p, u8p, C.c_uint32, C.c_uint32, u8p, u8p, u8p, C.c_int32]
    if hasattr(lib, "zk_plonk_quotient"):
        lib.zk_fr_coset_ntt.argtypes = [u8p, u8p, C.c_uint64, C.c_uint32, u8p, C.c_int, C.c_int32]
        lib.zk_plonk_circuit_create.argtypes = [C.POINTER(C.c_void_p), C.POINTER(zk_plonk_circuit_view), C.c_int32]
        lib.zk_plonk_circuit_destroy.argtypes = [C.c_void_p]
        lib.zk_plonk_circuit_destroy.restype = None
        lib.zk_plonk_circuit_info.argtypes = [C.c_void_p, C.POINTER(zk_plonk_circuit_plan)]
        lib.zk_plonk_quotient.argtypes = [C.c_void_p, u8p, C.POINTER(C.c_uint64), u8p, C.c_uint64, u8p, C.c_uint64, u8p, C.c_uint64, u8p, C.c_uint64, u8p,
                                          u8p, u8p, u8p]
    if hasattr(lib, "zk_plonk_open"):
        lib.zk_fr_poly_eval.argtypes = [u8p, u8p, C.c_uint64, C.c_uint64, u8p, C.c_int32]
        lib.zk_plonk_opening_create.argtypes = [C.POINTER(C.c_void_p), C.c_void_p, C.POINTER(zk_plonk_circuit_view), C.c_int32]
        lib.zk_plonk_opening_destroy.argtypes = [C.c_void_p]
        lib.zk_plonk_opening_destroy.restype = None
        lib.zk_plonk_opening_info.argtypes = [C.c_void_p, C.POINTER(zk_plonk_opening_plan)]
        lib.zk_plonk_evaluate.argtypes = [C.c_void_p, u8p, u8p, C.c_uint64, u8p, C.c_uint64, u8p, C.c_uint64, u8p, C.c_uint64, u8p]
        lib.zk_plonk_open.argtypes = [C.c_void_p, u8p, u8p, u8p, u8p, C.POINTER(C.c_uint64), u8p, C.c_uint64, u8p, C.c_uint64, u8p, C.c_uint64, u8p,
                                      u8p, u8p, u8p, u8p]
    if hasattr(lib, "zk_plonk_prove"):
        u32p = C.c_void_p
        lib.zk_keccak256.argtypes = [u8p, u8p, C.c_uint64]
        lib.zk_plonk_prover_create.argtypes = [C.POINTER(C.c_void_p), C.c_void_p, C.POINTER(zk_plonk_circuit_view), u32p, u32p, u32p, C.c_uint64, C.c_uint64,
                                               C.c_int32]
        lib.zk_plonk_prover_destroy.argtypes = [C.c_void_p]
        lib.zk_plonk_prover_destroy.restype = None
        lib.zk_plonk_prover_vkey.argtypes = [C.c_void_p, C.POINTER(zk_plonk_vkey)]
        lib.zk_plonk_prover_info.argtypes = [C.c_void_p, C.POINTER(zk_plonk_prover_plan)]
        lib.zk_plonk_prove.argtypes = [C.c_void_p, u8p, u8p, u8p, u8p]
        lib.zk_plonk_verify.argtypes = [C.c_void_p, C.POINTER(zk_plonk_vkey), u8p, u8p, u8p]
    if hasattr(lib, "zk_plonk_r1cs_create"):
        u32p = C.c_void_p
        lib.zk_plonk_r1cs_create.argtypes = [C.POINTER(C.c_void_p), C.POINTER(zk_r1cs_view), u8p, u8p, C.c_int32]
        lib.zk_plonk_r1cs_destroy.argtypes = [C.c_void_p]
        lib.zk_plonk_r1cs_destroy.restype = None
        lib.zk_plonk_r1cs_info.argtypes = [C.c_void_p, C.POINTER(zk_plonk_r1cs_plan)]
        lib.zk_plonk_r1cs_circuit.argtypes = [C.c_void_p, u8p, u32p, u32p, u32p]
        lib.zk_plonk_r1cs_extend.argtypes = [C.c_void_p, u8p, u8p, C.c_uint32]
        lib.zk_plonk_prover_create_r1cs.argtypes = [C.POINTER(C.c_void_p), C.c_void_p, C.c_void_p, u8p, C.c_int32]
        lib.zk_plonk_prove_r1cs.argtypes = [C.c_void_p, u8p, u8p, C.c_uint32, u8p]
    if hasattr(lib, "zk_plonk_prove_many"):
        lib.zk_plonk_prove_many.argtypes = [C.c_void_p, C.c_uint64, u8p, C.c_void_p, u8p, u8p, u8p]
        lib.zk_plonk_prove_r1cs_many.argtypes = [C.c_void_p, C.c_uint64, u8p, C.c_void_p, u8p, C.c_uint32, u8p]
        lib.zk_plonk_prover_commit_many.argtypes = [C.c_void_p, u8p, u8p, C.c_uint64]
        lib.zk_plonk_prover_many_info.argtypes = [C.c_void_p, C.POINTER(zk_plonk_prover_many_plan)]
    if hasattr(lib, "zk_plonk_verifier_create"):
        lib.zk_plonk_verifier_create.argtypes = [C.POINTER(C.c_void_p), C.POINTER(zk_plonk_vkey), C.c_int32]
        lib.zk_plonk_verifier_destroy.argtypes = [C.c_void_p]
        lib.zk_plonk_verifier_destroy.restype = None
        lib.zk_plonk_verifier_info.argtypes = [C.c_void_p, C.POINTER(zk_plonk_verifier_plan)]
        lib.zk_plonk_verifier_verify.argtypes = [C.c_void_p, u8p, u8p, C.c_uint64, u8p]
        lib.zk_plonk_verifier_challenges.argtypes = [C.c_void_p, u8p, u8p, C.c_uint64, u8p, u8p]
    if hasattr(lib, "zk_plonk_verifier_verify_batch"):
        lib.zk_plonk_verifier_verify_batch.argtypes = [C.c_void_p, u8p, u8p, C.c_uint64, u8p, u8p, C.POINTER(zk_plonk_batch_report)]
        lib.zk_plonk_verifier_batch_sums.argtypes = [C.c_void_p, u8p, u8p, C.c_uint64, u8p, u8p, C.c_uint64, C.POINTER(C.c_uint64)]
    if hasattr(lib, "zk_plonk_verifier_set_create"):
        lib.zk_plonk_verifier_set_create.argtypes = [C.POINTER(C.c_void_p), C.POINTER(C.POINTER(zk_plonk_vkey)), C.c_uint32, C.c_int32]
        lib.zk_plonk_verifier_set_destroy.argtypes = [C.c_void_p]
        lib.zk_plonk_verifier_set_destroy.restype = None
        lib.zk_plonk_verifier_set_info.argtypes = [C.c_void_p, C.POINTER(zk_plonk_verifier_set_plan)]
        lib.zk_plonk_verifier_set_verify.argtypes = [C.c_void_p, u8p, C.c_void_p, u8p, C.c_uint64, C.c_uint64, u8p]
        lib.zk_plonk_verifier_set_verify_batch.argtypes = [C.c_void_p, u8p, C.c_void_p, u8p, C.c_uint64, C.c_uint64, u8p, u8p,
                                                           C.POINTER(zk_plonk_set_batch_report)]
        lib.zk_plonk_verifier_set_batch_sums.argtypes = [C.c_void_p, u8p, C.c_void_p, u8p, C.c_uint64, C.c_uint64, u8p, u8p, C.c_uint64,
                                                         C.POINTER(C.c_uint64)]
    _LIB = lib
    return lib


def check(rc):
    if rc != 0:
        raise ZkHipError(load_library().zk_last_error().decode("utf-8", "replace"))


def _buf(b, nbytes=None):
    """bytes / bytearray / numpy uint8 -> contiguous numpy uint8 array (kept alive by caller)."""
    a = np.frombuffer(b, dtype=np.uint8) if not isinstance(b, np.ndarray) else np.ascontiguousarray(b).view(np.uint8).reshape(-1)
    if nbytes is not None and a.size != nbytes:
        raise ValueError("expected %d bytes, got %d" % (nbytes, a.size))
    return a


def _ptr(a):
    return C.c_void_p(a.ctypes.data)


def device_count():
    n = C.c_int(0)
    check(load_library().zk_device_count(C.byref(n)))
    return n.value


class PinnedBuffer:
    """Page-locked host memory from zk_host_alloc, exposed as a numpy uint8 array (`.array`).  A witness
    placed here is uploaded by the DMA engine directly (zk_prove_submit does not stage it)."""

    def __init__(self, nbytes):
        self._ptr = C.c_void_p()
        check(load_library().zk_host_alloc(C.byref(self._ptr), nbytes))
        self.nbytes = nbytes
        self.array = np.ctypeslib.as_array(C.cast(self._ptr, C.POINTER(C.c_uint8)), shape=(nbytes,))

    def free(self):
        if self._ptr is not None and self._ptr.value:
            self.array = None
            load_library().zk_host_free(self._ptr)
            self._ptr = C.c_void_p()

    __del__ = free


def _mul_vec(fn, a, b):
    a, b = _buf(a), _buf(b)
    assert a.size == b.size and a.size % 32 == 0
    out = np.empty_like(a)
    check(fn(_ptr(out), _ptr(a), _ptr(b), a.size // 32))
    return out.tobytes()


def fr_mul_vec(a, b):
    return _mul_vec(load_library().zk_fr_mul_vec, a, b)


def fq_mul_vec(a, b):
    return _mul_vec(load_library().zk_fq_mul_vec, a, b)


def fr_coef_accumulate(coefs, n_coefs, domain_size, wtns):
    """(a, b) = (A.w, B.w) from the packed coefficient records (zkey section 4 image incl. its u32 count) —
    src/groth16.cpp:62-85; a, b as numpy uint8 arrays, Montgomery form."""
    coefs, wtns = _buf(coefs), _buf(wtns)
    a = np.empty(domain_size * 32, dtype=np.uint8)
    b = np.empty(domain_size * 32, dtype=np.uint8)
    check(load_library().zk_fr_coef_accumulate(_ptr(a), _ptr(b), _ptr(coefs), n_coefs, domain_size, _ptr(wtns), wtns.size // 32))
    return a, b


def fr_ntt(data, inverse=False):
    a = _buf(data).copy()
    check(load_library().zk_fr_ntt(_ptr(a), a.size // 32, 1 if inverse else 0))
    return a.tobytes()


def fr_abc_to_h(a, b):
    a, b = _buf(a), _buf(b)
    out = np.empty_like(a)
    check(load_library().zk_fr_abc_to_h(_ptr(out), _ptr(a), _ptr(b), a.size // 32))
    return out.tobytes()


def msm_g1(bases, scalars):
    bases, scalars = _buf(bases), _buf(scalars)
    n = scalars.size // 32
    assert bases.size == n * 64
    out = np.zeros(64, dtype=np.uint8)
    check(load_library().zk_msm_g1(_ptr(out), _ptr(bases), _ptr(scalars), n))
    return out.tobytes()


def msm_g2(bases, scalars):
    bases, scalars = _buf(bases), _buf(scalars)
    n = scalars.size // 32
    assert bases.size == n * 128
    out = np.zeros(128, dtype=np.uint8)
    check(load_library().zk_msm_g2(_ptr(out), _ptr(bases), _ptr(scalars), n))
    return out.tobytes()


class zk_msm_sort_plan(C.Structure):
    _fields_ = [(k, C.c_uint32) for k in ("size", "c", "W", "sets", "nbuckets", "total_buckets", "table_mode", "batch")] + \
               [(k, C.c_uint64) for k in ("n", "max_entries", "entries")]


def msm_sort(scalars, n, window_bits=0, table_mode=0, batch=1, plan_only=False):
    """zk_msm_sort (include/zkhip.h): the digit recoding and bucket sort of `batch` vectors of n scalars each (n*batch*32
    bytes, LE standard form).  -> (plan as a dict, offsets uint32[total_buckets + 1], entries uint32[E]); plan_only=True
    fills the plan alone (no GPU needed; scalars may be None) and returns (plan, None, None)."""
    fn = getattr(load_library(), "zk_msm_sort", None)
    if fn is None:
        raise ZkHipError("zk_msm_sort is not in this build of libzkhip.so")
    plan = zk_msm_sort_plan()
    plan.size = C.sizeof(zk_msm_sort_plan)
    as_dict = lambda: {k: int(getattr(plan, k)) for k, _ in zk_msm_sort_plan._fields_ if k != "size"}
    check(fn(None, n, window_bits, int(table_mode), batch, C.byref(plan), None, None))
    if plan_only:
        return as_dict(), None, None
    sc = _buf(scalars)
    if sc.size != plan.n * 32:
        raise ValueError("scalars: %d bytes expected (batch x n x 32)" % (plan.n * 32))
    offsets = np.zeros(plan.total_buckets + 1, dtype=np.uint32)
    entries = np.zeros(plan.max_entries, dtype=np.uint32)
    check(fn(_ptr(sc), n, window_bits, int(table_mode), batch, C.byref(plan), _ptr(offsets), _ptr(entries)))
    return as_dict(), offsets, entries[:plan.entries].copy()


def proof_to_json(proof_bytes):
    p = zk_proof.from_buffer_copy(bytes(proof_bytes))
    lib = load_library()
    n = lib.zk_proof_to_json(C.byref(p), None, 0)
    buf = C.create_string_buffer(n + 1)
    lib.zk_proof_to_json(C.byref(p), buf, n + 1)
    return buf.value.decode()


def public_to_json(wtns_values_bytes, n_public):
    a = _buf(wtns_values_bytes)
    lib = load_library()
    n = lib.zk_public_to_json(_ptr(a), n_public, None, 0)
    buf = C.create_string_buffer(n + 1)
    lib.zk_public_to_json(_ptr(a), n_public, buf, n + 1)
    return buf.value.decode()


def synth_chain_g1(n, p0, q):
    """out[i] = P0 + i*Q on the GPU -> numpy uint8 [n*64] (affine Montgomery)."""
    out = np.zeros(n * 64, dtype=np.uint8)
    a, b = _buf(p0).copy(), _buf(q).copy()
    check(load_library().zk_synth_chain_g1(_ptr(out), n, _ptr(a), _ptr(b)))
    return out


def synth_chain_g2(n, p0, q):
    out = np.zeros(n * 128, dtype=np.uint8)
    a, b = _buf(p0).copy(), _buf(q).copy()
    check(load_library().zk_synth_chain_g2(_ptr(out), n, _ptr(a), _ptr(b)))
    return out


def _scalars_le(scalars):
    if isinstance(scalars, np.ndarray) and scalars.dtype == np.uint8:
        return np.ascontiguousarray(scalars)
    return np.frombuffer(b"".join(int(k).to_bytes(32, "little") for k in scalars), dtype=np.uint8).copy()


def fixed_base_g1(base, scalars):
    """[k*base for k in scalars] on the GPU -> numpy uint8 [n*64] (affine Montgomery; 0 -> all-zero).
    scalars: iterable of ints < 2^256, or uint8 array n*32 (LE standard form)."""
    sc = _scalars_le(scalars)
    n = sc.size // 32
    out = np.zeros(n * 64, dtype=np.uint8)
    b = _buf(base).copy()
    check(load_library().zk_fixed_base_g1(_ptr(out), _ptr(b), _ptr(sc), n))
    return out


def fixed_base_g2(base, scalars):
    sc = _scalars_le(scalars)
    n = sc.size // 32
    out = np.zeros(n * 128, dtype=np.uint8)
    b = _buf(base).copy()
    check(load_library().zk_fixed_base_g2(_ptr(out), _ptr(b), _ptr(sc), n))
    return out


def _lagrange(name, nb, points, log_n, device):
    pts = _buf(points)
    if pts.size % nb:
        raise ValueError("points: a multiple of %d bytes expected" % nb)
    out = np.zeros(nb << log_n, dtype=np.uint8)
    fn = getattr(load_library(), name, None)
    if fn is None:
        raise ZkHipError("%s is not in this build of libzkhip.so" % name)
    check(fn(_ptr(out), _ptr(pts) if pts.size else None, pts.size // nb, log_n, device))
    return out


def g1_lagrange(points, log_n, device=-1):
    """The inverse DFT over G1 points (zk_g1_lagrange): the first 2^log_n of `points` (n x 64 B affine Montgomery; missing
    ones count as infinity) -> numpy uint8 [2^log_n * 64], out_j = (1/n) sum_k w^(-jk) P_k.  With P_k = [tau^k]G this is
    one level of a .ptau's Lagrange section.  Raises ZkHipError naming the index of a point that is not on the curve."""
    return _lagrange("zk_g1_lagrange", 64, points, log_n, device)


def g2_lagrange(points, log_n, device=-1):
    return _lagrange("zk_g2_lagrange", 128, points, log_n, device)


def _scalar32(k):
    k = int(k)
    if not 0 <= k < 1 << 256:
        raise ValueError("scalar: 0 <= k < 2^256 expected")
    return np.frombuffer(k.to_bytes(32, "little"), dtype=np.uint8).copy()


def g1_scale(points, k, device=-1):
    """[k * P for P in points] on the GPU (zk_g1_scale): n x 64 B affine Montgomery in, numpy uint8 [n * 64] out, all-zero =
    infinity.  One scalar for all points (int, 0 <= k < r): the host splits it by BN254's endomorphism and recodes it once.
    Raises ZkHipError for k >= r and for a point that is not on the curve (the message names its index)."""
    pts = _buf(points)
    if pts.size % 64:
        raise ValueError("points: a multiple of 64 bytes expected")
    fn = getattr(load_library(), "zk_g1_scale", None)
    if fn is None:
        raise ZkHipError("zk_g1_scale is not in this build of libzkhip.so")
    out = np.zeros(pts.size, dtype=np.uint8)
    kk = _scalar32(k)
    check(fn(_ptr(out) if pts.size else None, _ptr(pts) if pts.size else None, pts.size // 64, _ptr(kk), device))
    return out


def g1_scale_plan(k):
    """zk_g1_scale_plan -> (digits_p, digits_phi): the joint signed-digit schedule the host makes of k, least significant
    first, sum 2^i (digits_p[i] + lambda digits_phi[i]) = k mod r.  No device is touched."""
    a, b = (C.c_int8 * ZK_SCALE_PLAN_MAX)(), (C.c_int8 * ZK_SCALE_PLAN_MAX)()
    n = C.c_uint32(0)
    kk = _scalar32(k)
    check(load_library().zk_g1_scale_plan(_ptr(kk), a, b, ZK_SCALE_PLAN_MAX, C.byref(n)))
    return list(a[:n.value]), list(b[:n.value])


def _mul_vec_points(name, nb, points, scalars, device):
    pts, sc = _buf(points), _scalars_le(scalars)
    if pts.size % nb:
        raise ValueError("points: a multiple of %d bytes expected" % nb)
    n = pts.size // nb
    if sc.size != 32 * n:
        raise ValueError("scalars: one of 32 bytes for each of the %d points expected" % n)
    out = np.zeros(pts.size, dtype=np.uint8)
    check(_need(name)(_ptr(out) if n else None, _ptr(pts) if n else None, _ptr(sc) if n else None, n, device))
    return out


def g1_mul_vec(points, scalars, device=-1):
    """[k_i * P_i] on the GPU (zk_g1_mul_vec): n x 64 B affine Montgomery points and n scalars (ints below r, or a uint8 array
    of n x 32 B little-endian) -> numpy uint8 [n * 64], all-zero = infinity.  Every lane splits its own scalar by BN254's
    endomorphism.  Raises ZkHipError naming the index of a scalar that is not below r or of a point that is not on the curve."""
    return _mul_vec_points("zk_g1_mul_vec", 64, points, scalars, device)


def g2_mul_vec(points, scalars, device=-1):
    """zk_g2_mul_vec: the same over n x 128 B G2 points, which must be in the order-r subgroup (the error names the index)."""
    return _mul_vec_points("zk_g2_mul_vec", 128, points, scalars, device)


def _power_scale(name, nb, points, base, first_exp, factor, device):
    pts = _buf(points)
    if pts.size % nb:
        raise ValueError("points: a multiple of %d bytes expected" % nb)
    out = np.zeros(pts.size, dtype=np.uint8)
    b, f = _scalar32(base), _scalar32(factor)
    check(_need(name)(_ptr(out) if pts.size else None, _ptr(pts) if pts.size else None, pts.size // nb, _ptr(b), first_exp, _ptr(f), device))
    return out


def g1_power_scale(points, base, first_exp=0, factor=1, device=-1):
    """[factor * base^(first_exp + i) * P_i] (zk_g1_power_scale): the scalars are made on the device.  base, factor: ints
    below r."""
    return _power_scale("zk_g1_power_scale", 64, points, base, first_exp, factor, device)


def g2_power_scale(points, base, first_exp=0, factor=1, device=-1):
    return _power_scale("zk_g2_power_scale", 128, points, base, first_exp, factor, device)


def glv_split(k):
    """zk_glv_split -> (k1, k2) with k = k1 + k2 lambda mod r and 0 < k1, k2 < 2^128: what a lane of zk_g*_mul_vec makes of
    its scalar.  No device is touched.  Raises ZkHipError for k >= r."""
    kk = _scalar32(k)
    a, b = np.zeros(16, dtype=np.uint8), np.zeros(16, dtype=np.uint8)
    check(_need("zk_glv_split")(_ptr(kk), _ptr(a), _ptr(b)))
    return int.from_bytes(a.tobytes(), "little"), int.from_bytes(b.tobytes(), "little")


def _need(name):
    fn = getattr(load_library(), name, None)
    if fn is None:
        raise ZkHipError("%s is not in this build of libzkhip.so" % name)
    return fn


def g2_in_subgroup(points, device=-1):
    """zk_g2_in_subgroup: n x 128 B affine Montgomery G2 points -> numpy uint8 [n], 1 = in the order-r subgroup of the twist
    (infinity: 1), 0 = on the twist but outside.  Raises ZkHipError naming the index of a point that is not on the twist."""
    pts = _buf(points)
    if pts.size % 128:
        raise ValueError("points: a multiple of 128 bytes expected")
    out = np.zeros(pts.size // 128, dtype=np.uint8)
    check(_need("zk_g2_in_subgroup")(_ptr(out) if out.size else None, _ptr(pts) if pts.size else None, out.size, device))
    return out


def _power_msm(name, nb, points, s, first_exp, device):
    pts = _buf(points)
    if pts.size % nb:
        raise ValueError("points: a multiple of %d bytes expected" % nb)
    out = np.zeros(nb, dtype=np.uint8)
    ss = _scalar32(s)
    check(_need(name)(_ptr(out), _ptr(pts) if pts.size else None, pts.size // nb, _ptr(ss), first_exp, device))
    return out.tobytes()


def g1_power_msm(points, s, first_exp=0, device=-1):
    """sum_i s^(first_exp + i) P_i over n x 64 B affine Montgomery G1 points (zk_g1_power_msm) -> 64 bytes, affine.  The
    scalars are made on the device.  s: int below r."""
    return _power_msm("zk_g1_power_msm", 64, points, s, first_exp, device)


def g2_power_msm(points, s, first_exp=0, device=-1):
    return _power_msm("zk_g2_power_msm", 128, points, s, first_exp, device)


def fr_power_dft(s, log_n, device=-1):
    """[sum_(i < 2^log_n) s^i w^(ij) for j < 2^log_n] (zk_fr_power_dft): the forward DFT of the powers of s, a list of ints,
    w the root of unity of fr_ntt."""
    out = np.zeros(32 << log_n, dtype=np.uint8)
    ss = _scalar32(s)
    check(_need("zk_fr_power_dft")(_ptr(out), _ptr(ss), log_n, device))
    raw = out.tobytes()
    return [int.from_bytes(raw[i:i + 32], "little") for i in range(0, len(raw), 32)]


def g1_mul(p, k):
    """k*P on the host (product code, 64-bit limbs): Curve::mulByScalar."""
    out = np.zeros(64, dtype=np.uint8)
    a, kk = _buf(p).copy(), np.frombuffer(int(k).to_bytes(32, "little"), dtype=np.uint8).copy()
    check(load_library().zk_g1_mul(_ptr(out), _ptr(a), _ptr(kk)))
    return out.tobytes()


def g2_mul(p, k):
    out = np.zeros(128, dtype=np.uint8)
    a, kk = _buf(p).copy(), np.frombuffer(int(k).to_bytes(32, "little"), dtype=np.uint8).copy()
    check(load_library().zk_g2_mul(_ptr(out), _ptr(a), _ptr(kk)))
    return out.tobytes()


def assemble(vk, partials, r=None, s=None):
    """Host-only final assembly (src/groth16.cpp:209-253) over the partial MSM sums of all shards.
    vk: dict with vk_alpha1, vk_beta1, vk_beta2, vk_delta1, vk_delta2 (bytes)."""
    keep = [_buf(vk[k]).copy() for k in ("vk_alpha1", "vk_beta1", "vk_beta2", "vk_delta1", "vk_delta2")]
    arr = (zk_msm_sums * len(partials))(*[zk_msm_sums.from_buffer_copy(bytes(p)) for p in partials])
    ra = np.frombuffer(int(r).to_bytes(32, "little"), dtype=np.uint8).copy() if r is not None else None
    sa = np.frombuffer(int(s).to_bytes(32, "little"), dtype=np.uint8).copy() if s is not None else None
    out = zk_proof()
    check(load_library().zk_assemble(*[_ptr(a) for a in keep], arr, len(partials),
                                     _ptr(ra) if ra is not None else None, _ptr(sa) if sa is not None else None, C.byref(out)))
    return bytes(out)
