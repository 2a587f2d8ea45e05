"""Which GPU tests launch each kernel of libenarf_paint.so and compare its output with a reference: the library's part of
the kernel registry, in the form of tests/kernel_coverage.py (keys: every kernel the library builds, demangled as its
`.kd` symbol prints; values: `module::function` of tests under tests/). tests/test_side_libraries_cpu.py requires the keys to equal
the built set, every entry to be non-empty and every named test to exist."""

_NS = "(anonymous namespace)::"
PAINT_KERNEL_TESTS = {
    f"{_NS}paint_shade_kernel(enarf_paint_shade_args)": [
        "test_gpu_paint::test_hand_written_fragments_match_the_referee",
        "test_gpu_paint::test_meshes_in_sine_colours_match_the_referee",
        "test_gpu_paint::test_white_lit_colours_give_the_rasteriser_image",
        "test_gpu_paint::test_label_mode_on_the_sphere_matches_the_referee",
        "test_gpu_paint::test_two_calls_are_bit_identical_and_an_empty_mesh_is_background",
        "test_gpu_paint::test_extract_mesh_returns_the_field_colour_of_every_vertex",
        "test_gpu_paint::test_render_colored_mesh_is_paint_mesh_of_its_own_pieces",
        "test_gpu_paint::test_mesh_turntable_equals_single_calls",
        "test_gpu_paint::test_part_animation_frames_are_composed_semantic_renders"],
}
GPU_TEST_MODULE = "test_gpu_paint"
