"""Which GPU tests launch each kernel of libenarf_sgrad.so and compare its output with a reference: the library's part of
the kernel registry, in the form of tests/kernel_coverage.py (keys: every kernel the library builds, demangled as its
`.kd` symbol prints; values: `module::function` of tests under tests/). tests/test_side_libraries_cpu.py requires the keys to equal
the built set, every entry to be non-empty and every named test to exist."""

_NS = "void (anonymous namespace)::"
_ARGS = "(enarf_sgrad_composite_bwd_args)"
# the shapes of tests/scene_cases.py reach every instantiation: K Nf = 2, 4, 15 (<1>), 65 (<2>), 256 (<4>), 512 (<8>)
_CASES = ["test_gpu_sgrad::test_cases_match_the_referee"]
SGRAD_KERNEL_TESTS = {
    f"{_NS}sgrad_composite_bwd_kernel<1>{_ARGS}": _CASES + [
        "test_gpu_sgrad::test_each_upstream_gradient_alone_and_want_writes_nothing_else",
        "test_gpu_sgrad::test_two_runs_are_bit_identical_one_frame_and_no_rays",
        "test_gpu_sgrad::test_render_scene_posable_two_avatars",
        "test_gpu_sgrad::test_one_avatar_scene_and_render_posable_meet_the_same_referee",
        "test_gpu_sgrad::test_fit_scene_descends",
        "test_gpu_sgrad::test_generator_scene_posable"],
    f"{_NS}sgrad_composite_bwd_kernel<2>{_ARGS}": _CASES + [
        "test_gpu_sgrad::test_two_runs_are_bit_identical_one_frame_and_no_rays",
        "test_gpu_sgrad::test_posable_composite_is_the_forward_and_the_raw_backward"],
    f"{_NS}sgrad_composite_bwd_kernel<4>{_ARGS}": _CASES,
    f"{_NS}sgrad_composite_bwd_kernel<8>{_ARGS}": _CASES,
}
GPU_TEST_MODULE = "test_gpu_sgrad"
