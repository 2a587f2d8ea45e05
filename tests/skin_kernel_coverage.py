"""Which GPU tests launch each kernel of libenarf_skin.so and compare its output with a reference: the library's part of
the kernel registry, in the form of tests/kernel_coverage.py (keys: every kernel the library builds, demangled as its
`.kd` symbol prints; values: `module::function` of tests under tests/). tests/test_side_libraries_cpu.py requires the keys to equal
the built set, every entry to be non-empty and every named test to exist. Every listed test runs K = 4 and K = 8."""

_NS = "void (anonymous namespace)::"
_WEIGHT_TESTS = ["test_gpu_skin::test_weights_on_scene_points_match_the_referee",
                 "test_gpu_skin::test_weights_on_explicit_vertices_tails_and_both_layouts",
                 "test_gpu_skin::test_weights_on_cube_faces_and_far_outside_every_cube",
                 "test_gpu_skin::test_six_coincident_parts_bit_for_bit",
                 "test_gpu_skin::test_skin_and_seg_agree_on_membership"]
_POSE_TESTS = ["test_gpu_skin::test_posing_matches_the_referee_to_one_fp32_step",
               "test_gpu_skin::test_posing_writes_into_a_slice_and_repeats_bit_for_bit"]
SKIN_KERNEL_TESTS = {
    f"{_NS}skin_weights_kernel<4>(enarf_skin_weights_args)": _WEIGHT_TESTS + ["test_gpu_skin::test_rigged_mesh_interface"],
    f"{_NS}skin_weights_kernel<8>(enarf_skin_weights_args)": _WEIGHT_TESTS,
    f"{_NS}skin_pose_kernel<4>(enarf_skin_pose_args)": _POSE_TESTS + ["test_gpu_skin::test_rigged_mesh_interface",
                                                                      "test_gpu_skin::test_mesh_animation_frames_are_single_renders"],
    f"{_NS}skin_pose_kernel<8>(enarf_skin_pose_args)": _POSE_TESTS,
}
GPU_TEST_MODULE = "test_gpu_skin"
