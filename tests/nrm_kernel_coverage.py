"""Which GPU tests launch each kernel of libenarf_nrm.so and compare its output with a reference: the library's part of the
kernel registry, in the form of tests/kernel_coverage.py (keys: every kernel the library builds, demangled as its `.kd`
symbol prints; values: `module::function` of tests under tests/). tests/test_side_libraries_cpu.py requires the keys to
equal the built set, every entry to be non-empty and every named test to exist."""

_NS = "(anonymous namespace)::"
NRM_KERNEL_TESTS = {
    f"{_NS}nrm_gradient_kernel(enarf_nrm_gradient_args)": [
        "test_gpu_nrm::test_gradient_matches_the_float64_referee",
        "test_gpu_nrm::test_density_matches_query_fwd",
        "test_gpu_nrm::test_points_outside_every_cube_get_exact_zeros",
        "test_gpu_nrm::test_two_runs_give_equal_bits"],
    f"{_NS}nrm_ray_kernel(enarf_nrm_ray_args)": [
        "test_gpu_nrm::test_ray_normals_match_the_referee",
        "test_gpu_nrm::test_two_runs_give_equal_bits"],
}
GPU_TEST_MODULE = "test_gpu_nrm"
