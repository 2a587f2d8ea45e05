"""Which GPU tests launch each kernel of libenarf_scene.so and compare its output with a reference: the library's part of
the kernel registry, in the form of tests/kernel_coverage.py (keys: every kernel the library builds, demangled as its
`.kd` symbol prints; values: `module::function` of tests under tests/). tests/test_side_libraries_cpu.py requires the keys to equal
the built set, every entry to be non-empty and every named test to exist."""

_NS = "void (anonymous namespace)::"
_ARGS = "(enarf_scene_composite_args)"
# the shapes of tests/scene_cases.py reach every instantiation: K Nf = 2, 4, 15 (<1>), 65 (<2>), 256 (<4>), 512 (<8>)
_CASES = ["test_gpu_scene::test_cases_match_the_referee"]
SCENE_KERNEL_TESTS = {
    f"{_NS}scene_composite_kernel<1>{_ARGS}": _CASES + [
        "test_gpu_scene::test_one_frame_without_its_axis_and_no_rays",
        "test_gpu_scene::test_one_avatar_is_render",
        "test_gpu_scene::test_avatars_side_by_side_are_the_sum_of_their_renders",
        "test_gpu_scene::test_the_nearer_avatar_covers_the_farther",
        "test_gpu_scene::test_generator_scene_and_its_animation"],
    f"{_NS}scene_composite_kernel<2>{_ARGS}": _CASES + [
        "test_gpu_scene::test_two_calls_are_bit_identical_and_want_writes_nothing_else"],
    f"{_NS}scene_composite_kernel<4>{_ARGS}": _CASES,
    f"{_NS}scene_composite_kernel<8>{_ARGS}": _CASES,
}
GPU_TEST_MODULE = "test_gpu_scene"
