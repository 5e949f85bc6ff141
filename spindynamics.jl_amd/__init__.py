"""spindynamics.jl_amd -- host-side mirror of the SpinDynamics.jl interface for the
H|psi> hot path, backed by libspindyn.so (hand-written HIP for gfx950 / MI355X).

The directory name contains a dot, so load the package through
`__graft_entry__.load_package()` (registers it as `spindynamics_jl_amd`).
Importing does not need a GPU; creating a context / model does, and raises when
the library or a device is missing -- there is no CPU fallback.
"""
from ._lib import (ArgumentError, Context, check, DimensionMismatch, SpinDynError, ZeroNormError, default_context, lib,
                   LIB_PATH, PROTOTYPES)
from .model import Model, XXZChain, build_model, long_range_hopping, momenta, nn_hopping
from .hamiltonian import (Sminus_q_vector, Splus_q_vector, Sz_q_vector, apply_H, apply_rescaled_H, bit_at, cheb_step,
                          create_spin_operator, flip_bits, sz_value)
from .solvers import (chebyshev_coeffs, chebyshev_terms, chebyshev_time_evolve, compute_chebyshev_moments, estimate_energy_bounds,
                      get_kernel, get_rescaling_params, kpm_reconstruct, kpm_sqw, kpm_sqw_transverse, kpm_sw,
                      krylov_time_evolve, lanczos_extremal, lanczos_groundstate, lanczos_sqw, lanczos_sqw_transverse,
                      lanczos_tridiag, rescaling_from_bounds, spectral_from_tridiagonal, symtridiag_eig,
                      kpm_correlation_matrix, kpm_reconstruct_signed, kpm_site_moments, kpm_sqw_sites, site_project,
                      lanczos_eigenpairs, lowest_eigenpairs, spectral_gap, sym_eig)
from .typicality import (chebyshev_imag_coeffs, current_expectation, dqt_sample, energy_current, energy_current_expectation,
                         energy_current_terms, spin_current, thermal_energy, thermal_state, typicality_correlation_function)
from .observables import (bond_energies, bond_operator, connected_correlations, correlation_matrix, dimer_correlation_matrix,
                          dimer_structure_factor, magnetization_per_site, model_bonds, momentum_distribution,
                          static_structure_factor, structure_factor_Sq)
from .symmetry import (is_symmetric, lowest_level, lowest_levels, momentum_weights, permutation_compose, permutation_inverse, permute_sites,
                       quantum_numbers, reflect, spin_flip, subsystem_permutation, symmetric_operator, symmetry_apply,
                       symmetry_combine, symmetry_overlaps, symmetry_project, translate)
from .operators import (Term, chirality_correlations, chirality_terms, hamiltonian_terms, multi_spin_expectation,
                        op_string, operator_adjoint, operator_apply, operator_check, operator_expectations,
                        operator_groundstate, operator_hamiltonian, operator_is_hermitian, operator_simplify, pack_terms,
                        scalar_chirality, string_order, string_order_terms)
from .statistics import (counting_statistics, cut_counting_statistics, inverse_participation_ratio, magnetization_cumulants,
                         most_probable_configuration, number_entropy, participation_entropy, sample_configurations,
                         snapshot_spins)
from .entanglement import (CutBlock, cut_blocks, cut_gram, cut_plan_info, dense_density_matrix, entanglement_entropy,
                           entanglement_profile, entanglement_spectrum, entropy_from_spectrum, logarithmic_negativity,
                           mutual_information, partial_transpose, reduced_density_matrix, schmidt_gap, spectrum_from_blocks,
                           subsystem_density_matrix, subsystem_entropy, subsystem_gram, subsystem_spectrum,
                           symmetry_resolved_entanglement, symmetry_resolved_from_spectrum, two_site_density_matrix)
from .driven import (DiagonalDrive, HoppingDrive, current_drive, diagonal_apply, diagonal_expectation, drive_check,
                     drive_expectation, driven_apply, driven_time_evolve, exchange_drive, field_drive, gradient_drive,
                     hopping_apply, instantaneous_energy, magnus_schedule, peierls_drives, peierls_functions,
                     piecewise_schedule, stage_evolve, zz_drive)
from . import initial_states
from .initial_states import domain_wall_state, neel_state, polarized_state, polarized_state_with_flips
from .api import dynamical_structure_factor, groundstate, structure_factor, time_evolve
from .dist import ShardedOperator, kpm_sqw_replicas

__all__ = [n for n in dir() if not n.startswith("_")]
