"""MI355X-native backend for the BN256 MSM / Fr-NTT hot path of the PSE halo2 prover.

Host-side mirror of ``halo2_proofs::arithmetic`` (``best_multiexp``, ``best_fft``, ``eval_polynomial``) and of the
``EvaluationDomain`` / ``ParamsKZG`` steps around them, over the C ABI of ``libhalo2_mi355x.so``.

The sources live in ``halo2-experiments_amd/`` (the directory name the project layout prescribes; not a valid
Python identifier): this package is the importable name, and its ``__path__`` points there, so every submodule
(``_header``, ``_lib``, ``_marshal``, ``arithmetic``, ``batch_verifier``, ``bn256``, ``device_pairing``, ``device_transcript``, ``domain``, ``gwc``, ``keygen``, ``kzg``, ``ledger``, ``mock_prover``, ``openings``, ``pairing``, ``poseidon``, ``proof_layout``, ``prover``, ``replay``, ``sharding``, ``shplonk``, ``solvency``, ``synthesis``, ``transcript``, ``verifier``) is an ordinary module of this package
with an ordinary ``__spec__`` / ``__file__``.
"""
import os as _os

__path__.append(_os.path.join(_os.path.dirname(_os.path.dirname(_os.path.abspath(__file__))), "halo2-experiments_amd"))

from . import _lib  # noqa: F401
from .arithmetic import (bases_info, batch_invert, best_fft, best_multiexp, best_multiexp_batch, best_multiexp_submit,  # noqa: F401
                         best_multiexp_wait, eval_polynomial, g1_check, g1_check_host, g1_compress, g1_compress_host,
                         g1_decompress, g1_decompress_host, g1_fft, g1_fft_host, g1_fixed_base_mul, g_to_lagrange, grand_product, grand_product_batch, grand_sum_batch, kate_division,
                         kate_division_batch,
                         linear_combination, linear_combination_batch, logup_multiplicities, msm_stats, permute_expression_pair, permute_expression_pairs, random_fr, register_bases,
                         release_bases)
from .batch_verifier import BatchVerifier, verify_each, verify_proofs  # noqa: F401
from .domain import EvaluationDomain  # noqa: F401
from .keygen import (ProvingKey, VerifyingKey, copy_pairs, keygen_pk, keygen_vk, permutation_cells_dev,  # noqa: F401
                     permutation_columns_dev)
from .ledger import (LedgerProof, LedgerStatement, ledger_eta, ledger_gamma, ledger_openings, ledger_order, ledger_statement,  # noqa: F401
                     prove_ledger, verify_ledger, verify_ledger_user, verify_ledger_users)
from .mock_prover import MockProver, MockResult, NotSatisfied  # noqa: F401
from .openings import OpeningTable, open_all, open_all_ints, open_at, verify_opening, verify_openings  # noqa: F401
from .pairing import pairing_check  # noqa: F401
from .poseidon import MerkleSumTree, MerkleTree, Spec, poseidon_hash, poseidon_hash_host, update_plan  # noqa: F401
from .prover import create_proof, create_proof_multi, create_proofs  # noqa: F401
from .shplonk import construct_intermediate_sets, create_openings, set_quotient, set_quotient_batch, set_quotient_ints  # noqa: F401
from .solvency import BalanceProof, prove_balances, user_openings, verify_balances, verify_user, verify_users  # noqa: F401
from .synthesis import (MerkleSumTreeLayout, MerkleTreeV3Layout, PoseidonCircuitLayout, RangeCheckLayout, SortedColumnLayout, merkle_sum_witness,  # noqa: F401
                        merkle_sum_witness_host, merkle_witness, merkle_witness_host, permutation_columns, poseidon_circuit_witness,
                        poseidon_circuit_witness_host, range_c_layout, range_witness, range_witness_host, sorted_c_layout, sorted_witness,
                        sorted_witness_host)
from .transcript import Blake2bRead, Blake2bWrite, KeccakRead, KeccakWrite, keccak256  # noqa: F401
from .verifier import verify_proof, verify_proof_multi  # noqa: F401

__all__ = ["eval_polynomial", "best_multiexp", "best_multiexp_batch", "best_multiexp_submit", "best_multiexp_wait", "best_fft",
           "register_bases", "release_bases", "bases_info", "g1_fixed_base_mul", "g1_fft", "g1_fft_host", "g1_compress", "g1_compress_host",
           "g1_decompress", "g1_decompress_host", "g1_check", "g1_check_host", "g_to_lagrange", "msm_stats", "kate_division", "kate_division_batch", "grand_product",
           "grand_product_batch", "grand_sum_batch", "logup_multiplicities", "batch_invert",
           "linear_combination", "random_fr", "permute_expression_pair", "permute_expression_pairs", "EvaluationDomain",
           "Spec", "poseidon_hash", "poseidon_hash_host", "update_plan", "MerkleSumTree", "MerkleTree", "MerkleSumTreeLayout", "merkle_sum_witness",
           "merkle_sum_witness_host", "permutation_columns", "MerkleTreeV3Layout", "PoseidonCircuitLayout", "merkle_witness",
           "merkle_witness_host", "poseidon_circuit_witness", "poseidon_circuit_witness_host", "copy_pairs", "permutation_cells_dev",
           "permutation_columns_dev", "keygen_vk", "keygen_pk", "VerifyingKey", "ProvingKey",
           "create_proof", "create_proof_multi", "create_proofs", "verify_proof", "verify_proof_multi", "Blake2bWrite", "Blake2bRead", "KeccakWrite", "KeccakRead", "keccak256", "pairing_check", "construct_intermediate_sets",
           "set_quotient", "set_quotient_batch", "set_quotient_ints", "create_openings", "linear_combination_batch", "MockProver", "MockResult", "NotSatisfied", "BatchVerifier", "verify_proofs", "verify_each",
           "OpeningTable", "open_all", "open_all_ints", "open_at", "verify_opening", "verify_openings",
           "RangeCheckLayout", "range_witness", "range_witness_host", "range_c_layout", "BalanceProof", "prove_balances", "verify_balances",
           "user_openings", "verify_user", "verify_users",
           "LedgerProof", "LedgerStatement", "ledger_statement", "prove_ledger", "verify_ledger", "ledger_gamma", "ledger_eta", "ledger_openings", "verify_ledger_user", "verify_ledger_users",
           "SortedColumnLayout", "sorted_witness", "sorted_witness_host", "sorted_c_layout", "ledger_order"]
