"""rapidsnark-old_amd — MI355X-native Groth16 hot path (drop-in for rapidsnark's prove()).

Python side = thin ctypes binding over the C-ABI in include/zkhip.h (libzkhip.so) plus a
mirror of the reference's binfile/zkey/wtns readers.  There is no Python/CPU compute
fallback: if libzkhip.so is missing or HIP has no device, calls raise.
"""
import os as _os
_os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")      # before the first HIP call of the process (lib.py: load_library)
from .binfile import BinFile, open_existing            # noqa: F401
from .zkey import ZkeyHeader, load_zkey_header, zkey_contribute      # noqa: F401
from .wtns import WtnsHeader, load_wtns_header          # noqa: F401
from .lib import (ZkHipError, load_library, library_path, fr_mul_vec, fq_mul_vec, fr_ntt, fr_coef_accumulate,   # noqa: F401
                  fr_abc_to_h, msm_g1, msm_g2, proof_to_json, public_to_json, device_count,
                  synth_chain_g1, synth_chain_g2, fixed_base_g1, fixed_base_g2, g1_lagrange, g2_lagrange, g1_scale, g1_scale_plan, g1_mul, g2_mul, assemble, PinnedBuffer,
                  g2_in_subgroup, g1_power_msm, g2_power_msm, fr_power_dft,
                  g1_mul_vec, g2_mul_vec, g1_power_scale, g2_power_scale, glv_split, msm_sort)
from .prover import Prover, MultiProver, prove_files                 # noqa: F401
from .r1cs import R1cs, R1csReport, write_r1cs                      # noqa: F401
from .ptau import PtauFile, PtauReport, groth16_setup, prepare_phase2, ptau_check, ptau_check_sizes, write_trapdoor_ptau, ptau_new, ptau_contribute, ptau_contribute_sizes      # noqa: F401
from .zkverify import ZkeyVerifyReport, zkey_verify, zkey_verify_sizes      # noqa: F401
from .verify import VerificationKey, VerificationKeySet, pairing, pairing_last_path, groth16_verify, load_proof, load_public      # noqa: F401
from .kzg import Kzg, fr_poly_divide                                  # noqa: F401
from .frscan import fr_batch_inverse, fr_prefix_product, fr_grand_product, plonk_permutation_product      # noqa: F401
from .plonk import PlonkCircuit, PlonkOpening, fr_coset_ntt, fr_poly_eval        # noqa: F401
from .plonk import PlonkProver, PlonkProof, PlonkVKey, PlonkR1cs, PlonkVerifier, PlonkVerifierSet, plonk_verify, keccak256        # noqa: F401
from . import synth                                     # noqa: F401
from .dist import gather_partials, ShardedChain                        # noqa: F401
