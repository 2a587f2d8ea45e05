"""Which GPU tests launch each kernel of libenarf_anim.so and compare its output with a reference: the library's part of
the kernel registry, in the form of tests/kernel_coverage.py (keys: every kernel the library builds, demangled as its
`.kd` symbol prints; values: `module::function` of tests under tests/). tests/test_side_libraries_cpu.py requires the keys to equal
the built set, every entry to be non-empty and every named test to exist, as tests/test_libraries_cpu.py does for the rows
of enarf_gan_amd.build.LIBRARIES."""

_NS = "(anonymous namespace)::"
ANIM_KERNEL_TESTS = {
    f"{_NS}anim_pose_kernel({_NS}PoseArgs)": [
        "test_gpu_anim::test_pose_kernel_matches_referee_and_golden", "test_gpu_anim::test_pose_kernel_with_orbit",
        "test_gpu_anim::test_pose_kernel_chain_of_64_and_single_joint", "test_gpu_anim::test_pose_kernel_null_outputs_are_not_written",
        "test_gpu_anim::test_two_runs_give_identical_bits"],
    f"{_NS}anim_compose_kernel({_NS}ComposeArgs)": [
        "test_gpu_anim::test_compose_matches_restatement_byte_for_byte", "test_gpu_anim::test_compose_on_decisions",
        "test_gpu_anim::test_compose_into_unaligned_slices_and_from_unaligned_inputs",
        "test_gpu_anim::test_render_animation_chunks_match_forward_on_the_same_chunks",
        "test_gpu_anim::test_render_animation_one_frame_per_batch_matches_single_frame_calls"],
}
GPU_TEST_MODULE = "test_gpu_anim"
