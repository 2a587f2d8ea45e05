"""Which GPU tests launch each kernel of libenarf_pgrad.so and compare its output with a reference: the library's part of
the kernel registry, in the form of tests/kernel_coverage.py (keys: every kernel the library builds, demangled as its
`.kd` symbol prints; values: `module::function` of tests under tests/). tests/test_side_libraries_cpu.py requires the keys to equal
the built set, every entry to be non-empty and every named test to exist. Both kernels run in every call."""

_NS = "(anonymous namespace)::"
_TESTS = ["test_gpu_pgrad::test_gradients_match_the_float64_referee",
          "test_gpu_pgrad::test_one_upstream_gradient_missing",
          "test_gpu_pgrad::test_points_outside_every_cube_get_exact_zeros",
          "test_gpu_pgrad::test_two_runs_give_equal_bits",
          "test_gpu_pgrad::test_query_posable_forward_and_pose_gradients"]
PGRAD_KERNEL_TESTS = {
    f"{_NS}pgrad_query_kernel(enarf_pgrad_query_args, int)": _TESTS,
    f"{_NS}pgrad_finish_kernel(double const*, float*, int, int)": _TESTS,
}
GPU_TEST_MODULE = "test_gpu_pgrad"
