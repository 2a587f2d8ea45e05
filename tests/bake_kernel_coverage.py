"""Which GPU tests launch each kernel of libenarf_bake.so and compare its output with a reference: the library's part of
the kernel registry, in the form of tests/kernel_coverage.py (keys: every kernel the library builds, demangled as its
`.kd` symbol prints; values: `module::function` of tests under tests/). tests/test_side_libraries_cpu.py requires the keys to equal
the built set, every entry to be non-empty and every named test to exist."""

_NS = "(anonymous namespace)::"
BAKE_KERNEL_TESTS = {
    f"{_NS}bake_points_kernel(enarf_bake_points_args, {_NS}Layout)": [
        "test_gpu_bake::test_bake_points_match_the_referee_on_every_texel",
        "test_gpu_bake::test_bands_of_rows_stitch_to_the_whole_atlas",
        "test_gpu_bake::test_two_calls_are_bit_identical_and_an_empty_mesh_is_empty",
        "test_gpu_bake::test_bake_texture_of_the_field_is_the_query_at_the_texel_points"],
    f"{_NS}bake_resolve_kernel(enarf_bake_resolve_args)": [
        "test_gpu_bake::test_bake_resolve_matches_the_referee",
        "test_gpu_bake::test_two_calls_are_bit_identical_and_an_empty_mesh_is_empty",
        "test_gpu_bake::test_bake_texture_of_the_parts_is_part_labels_through_the_palette"],
    f"{_NS}bake_shade_kernel(enarf_bake_shade_args, {_NS}Layout)": [
        "test_gpu_bake::test_hand_written_fragments_match_the_referee",
        "test_gpu_bake::test_the_textured_sphere_matches_the_referee",
        "test_gpu_bake::test_no_colour_bleeds_from_one_face_to_another",
        "test_gpu_bake::test_an_affine_colour_is_reproduced_up_to_the_edges",
        "test_gpu_bake::test_a_texture_resolves_detail_vertex_colours_cannot",
        "test_gpu_bake::test_two_calls_are_bit_identical_and_an_empty_mesh_is_empty",
        "test_gpu_bake::test_render_textured_mesh_is_paint_textured_mesh_of_its_own_pieces",
        "test_gpu_bake::test_a_frame_of_the_textured_animation_is_skin_mesh_and_paint_textured_mesh"],
}
GPU_TEST_MODULE = "test_gpu_bake"
