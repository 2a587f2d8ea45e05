"""Which GPU tests launch each kernel of libenarf_geom.so and compare its output with a reference: the library's part of
the kernel registry, in the form of tests/kernel_coverage.py (keys: every kernel the library builds, demangled as its
`.kd` symbol prints; values: `module::function` of tests under tests/). tests/test_side_libraries_cpu.py requires the keys to equal
the built set, every entry to be non-empty and every named test to exist."""

_NS = "(anonymous namespace)::"
_ERR_TESTS = ["test_gpu_geom::test_depth_error_matches_the_referee_and_repeats_bit_for_bit",
              "test_gpu_geom::test_depth_error_over_many_workgroups_and_non_finite_values",
              "test_gpu_geom::test_inverse_depth_error_is_the_depth_error_of_forward"]
GEOM_KERNEL_TESTS = {
    f"{_NS}geom_buffers_kernel(enarf_geom_buffers_args)": [
        "test_gpu_geom::test_hand_written_buffers_match_the_referee",
        "test_gpu_geom::test_scenes_match_the_referee",
        "test_gpu_geom::test_two_calls_are_bit_identical_and_want_writes_nothing_else",
        "test_gpu_geom::test_render_geometry_is_geometry_buffers_of_forward",
        "test_gpu_geom::test_geometry_animation_frames_are_single_renders",
        "test_gpu_geom::test_inverse_zbuf_gives_back_the_zbuf"],
    f"{_NS}geom_err_partial_kernel(float const*, float const*, float const*, long long, float, long long*)": _ERR_TESTS,
    f"{_NS}geom_err_finish_kernel(long long const*, int, long long, long long*)": _ERR_TESTS,
}
GPU_TEST_MODULE = "test_gpu_geom"
