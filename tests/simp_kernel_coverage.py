"""Which GPU tests launch each kernel of libenarf_simp.so and compare its output with a reference: the library's part of
the kernel registry, in the form of tests/kernel_coverage.py (keys: every kernel the library builds, demangled as its
`.kd` symbol prints; values: `module::function` of tests under tests/). tests/test_side_libraries_cpu.py requires the keys to equal
the built set, every entry to be non-empty and every named test to exist. test_every_case_matches_the_referee runs both
placements on every hand mesh and on the sphere at four cell sizes and compares every output of the call."""

_NS = "(anonymous namespace)::"
_BOTH = ["test_gpu_simp::test_every_case_matches_the_referee",
         "test_gpu_simp::test_two_calls_are_bit_identical_and_an_empty_mesh_is_empty",
         "test_gpu_simp::test_an_origin_below_the_minimum_shifts_the_cells_as_the_referee_says"]
_QUADRIC = _BOTH + ["test_gpu_simp::test_a_target_triangle_count_is_met_and_one_step_finer_exceeds_it",
                    "test_gpu_simp::test_extract_mesh_with_simplify_cell_is_simplify_mesh_of_extract_mesh",
                    "test_gpu_simp::test_a_simplified_rig_is_made_of_its_own_pieces_and_round_trips_through_glb"]
SIMP_KERNEL_TESTS = {
    f"{_NS}simp_key_kernel(enarf_simp_keys_args)": _QUADRIC,
    f"{_NS}simp_corner_kernel(enarf_simp_corners_args)": _QUADRIC,
    f"void {_NS}simp_place_kernel<true>(enarf_simp_place_args)": _QUADRIC,
    f"void {_NS}simp_place_kernel<false>(enarf_simp_place_args)": _BOTH,
}
GPU_TEST_MODULE = "test_gpu_simp"
