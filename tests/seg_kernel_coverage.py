"""Which GPU tests launch each kernel of libenarf_seg.so and compare its output with a reference: the library's part of
the kernel registry, in the form of tests/kernel_coverage.py (keys: every kernel the library builds, demangled as its
`.kd` symbol prints; values: `module::function` of tests under tests/). tests/test_side_libraries_cpu.py requires the keys to equal
the built set, every entry to be non-empty and every named test to exist, as tests/test_libraries_cpu.py does for the rows
of enarf_gan_amd.build.LIBRARIES."""

_NS = "(anonymous namespace)::"
SEG_KERNEL_TESTS = {
    f"{_NS}seg_label_kernel(enarf_seg_label_args)": [
        "test_gpu_seg::test_labels_on_the_fine_samples_of_a_march", "test_gpu_seg::test_explicit_points_tails_and_both_layouts",
        "test_gpu_seg::test_no_points_and_points_outside_every_cube",
        "test_gpu_seg::test_points_on_cube_faces_against_the_referee_and_the_query_kernel",
        "test_gpu_seg::test_extract_mesh_returns_one_label_per_vertex"],
    f"{_NS}seg_composite_kernel(enarf_seg_composite_args)": [
        "test_gpu_seg::test_composite_of_a_march_matches_the_referee", "test_gpu_seg::test_composite_sample_counts_and_edge_rays",
        "test_gpu_seg::test_render_entire_img_semantic_map_is_the_composite_of_its_own_taps",
        "test_gpu_seg::test_render_part_map_shapes_and_dtypes"],
}
GPU_TEST_MODULE = "test_gpu_seg"
