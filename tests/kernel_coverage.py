"""Which GPU tests launch each kernel instantiation of each HIP library and compare its output with a reference.

One map per row of enarf_gan_amd.build.LIBRARIES (LIBRARY_KERNEL_TESTS at the end; KERNEL_TESTS is libenarf_hip.so's).
Keys: every instantiation the library builds, demangled as its `.kd` (kernel descriptor) symbol prints
(tools/check_mfma_chains.kernel_symbols); values: `module::function` of tests under tests/. A kernel-trace run of the GPU
suite (rocprofv3 --kernel-trace) is what these entries were read from. tests/test_libraries_cpu.py requires the keys to
equal the built set, every entry to be non-empty and every named test to exist: a new template instantiation needs a test
named here before the CPU suite passes.
"""

_UPF = "enarf::UpfirParams"
_RA = "enarf_render_args"
_QA = "enarf_query_args, int, int"
_SAMPLER = "float const*, float const*, float*, int, int, long long, enarf::SamplerCfg"
_PACK = "float const*, float*, int, int, int"
_BIAS_ACT = "float const*, float const*, float const*, float*, long long, int, long long, float, float"

KERNEL_TESTS = {
    # ---- 2-D GAN ops (csrc/enarf_gan_ops.hip)
    f"void enarf::bias_act_kernel<1>({_BIAS_ACT})": [
        "test_gpu_gan2d::test_fused_leaky_relu_forward_backward_and_second_derivative",
        "test_gpu_gan2d::test_fused_leaky_relu_grid_stride_loop",
        "test_gpu_gan2d::test_fused_leaky_relu_misaligned_many_channels_and_slopes"],
    f"void enarf::bias_act_kernel<4>({_BIAS_ACT})": [
        "test_gpu_gan2d::test_fused_leaky_relu_forward_backward_and_second_derivative",
        "test_gpu_gan2d::test_fused_leaky_relu_grid_stride_loop",
        "test_gpu_gan2d::test_fused_leaky_relu_misaligned_many_channels_and_slopes"],
    f"void enarf::upfirdn2d_kernel<2, 1, 4, 4, 16, 1, false>({_UPF})": [
        "test_gpu_gan2d::test_upfirdn2d_matches_restatement", "test_gpu_gan2d::test_upfirdn2d_asymmetric_filters",
        "test_gpu_gan2d::test_upfirdn2d_backward_and_second_derivative_asymmetric", "test_gpu_gan2d::test_upfirdn2d_plan_boundaries",
        "test_gpu_gan2d::test_upfirdn2d_pipeline_planes"],
    f"void enarf::upfirdn2d_kernel<2, 1, 0, 0, 16, 1, false>({_UPF})": [
        "test_gpu_gan2d::test_upfirdn2d_matches_restatement", "test_gpu_gan2d::test_upfirdn2d_asymmetric_filters",
        "test_gpu_gan2d::test_upfirdn2d_backward_and_second_derivative_asymmetric", "test_gpu_gan2d::test_upfirdn2d_plan_boundaries",
        "test_gpu_gan2d::test_upfirdn2d_pipeline_planes"],
    f"void enarf::upfirdn2d_kernel<1, 2, 4, 4, 8, 1, false>({_UPF})": [
        "test_gpu_gan2d::test_upfirdn2d_matches_restatement", "test_gpu_gan2d::test_upfirdn2d_asymmetric_filters",
        "test_gpu_gan2d::test_upfirdn2d_backward_and_second_derivative_asymmetric", "test_gpu_gan2d::test_upfirdn2d_plan_boundaries",
        "test_gpu_gan2d::test_upfirdn2d_pipeline_planes"],
    f"void enarf::upfirdn2d_kernel<1, 2, 0, 0, 8, 1, false>({_UPF})": [
        "test_gpu_gan2d::test_upfirdn2d_matches_restatement", "test_gpu_gan2d::test_upfirdn2d_asymmetric_filters",
        "test_gpu_gan2d::test_upfirdn2d_backward_and_second_derivative_asymmetric", "test_gpu_gan2d::test_upfirdn2d_plan_boundaries",
        "test_gpu_gan2d::test_upfirdn2d_pipeline_planes"],
    f"void enarf::upfirdn2d_kernel<1, 1, 4, 4, 8, 2, true>({_UPF})": [
        "test_gpu_gan2d::test_upfirdn2d_matches_restatement", "test_gpu_gan2d::test_upfirdn2d_asymmetric_filters",
        "test_gpu_gan2d::test_upfirdn2d_plan_boundaries", "test_gpu_gan2d::test_upfirdn2d_pipeline_planes"],
    f"void enarf::upfirdn2d_kernel<1, 1, 4, 4, 8, 2, false>({_UPF})": [
        "test_gpu_gan2d::test_upfirdn2d_matches_restatement", "test_gpu_gan2d::test_upfirdn2d_asymmetric_filters",
        "test_gpu_gan2d::test_upfirdn2d_plan_boundaries", "test_gpu_gan2d::test_upfirdn2d_pipeline_planes"],
    f"void enarf::upfirdn2d_kernel<1, 1, 4, 4, 16, 1, true>({_UPF})": [
        "test_gpu_gan2d::test_upfirdn2d_plan_boundaries", "test_gpu_gan2d::test_upfirdn2d_pipeline_planes"],
    f"void enarf::upfirdn2d_kernel<1, 1, 4, 4, 16, 1, false>({_UPF})": [
        "test_gpu_gan2d::test_upfirdn2d_matches_restatement", "test_gpu_gan2d::test_upfirdn2d_asymmetric_filters",
        "test_gpu_gan2d::test_upfirdn2d_backward_and_second_derivative_asymmetric", "test_gpu_gan2d::test_upfirdn2d_plan_boundaries",
        "test_gpu_gan2d::test_upfirdn2d_pipeline_planes", "test_gpu_gan2d::test_discriminator_matches_reference_golden"],
    f"void enarf::upfirdn2d_kernel<1, 1, 0, 0, 16, 1, false>({_UPF})": [
        "test_gpu_gan2d::test_upfirdn2d_matches_restatement", "test_gpu_gan2d::test_upfirdn2d_asymmetric_filters",
        "test_gpu_gan2d::test_upfirdn2d_backward_and_second_derivative_asymmetric", "test_gpu_gan2d::test_upfirdn2d_plan_boundaries",
        "test_gpu_gan2d::test_upfirdn2d_pipeline_planes"],
    # ---- tri-plane sampler (csrc/enarf_sampler.hip)
    f"void enarf::pack_kernel<8>({_PACK})": [
        "test_gpu_parity::test_sampler_fast_path_vs_oracle", "test_gpu_parity::test_sampler_padding_modes_vs_torch",
        "test_gpu_sampler_referee::test_sampler_forward_on_decisions"],
    f"void enarf::pack_kernel<16>({_PACK})": [
        "test_gpu_parity::test_sampler_fast_path_vs_oracle", "test_gpu_parity::test_sampler_fast_path_channel_widths_at_tile_edges",
        "test_gpu_sampler_referee::test_sampler_forward_on_decisions"],
    f"void enarf::pack_kernel<32>({_PACK})": [
        "test_gpu_parity::test_sampler_fast_path_vs_oracle", "test_gpu_parity::test_render_vs_oracle_and_golden",
        "test_gpu_parity::test_query_vs_oracle_and_golden",
        "test_gpu_sampler_referee::test_sampler_forward_on_decisions",
        "test_gpu_sampler_referee::test_sampler_backward_fast_path_on_decisions"],
    f"void enarf::pack_kernel<64>({_PACK})": [
        "test_gpu_parity::test_sampler_fast_path_vs_oracle", "test_gpu_parity::test_sampler_fast_path_channel_widths_at_tile_edges",
        "test_gpu_sampler_referee::test_sampler_forward_on_decisions"],
    f"void enarf::sample_fwd_cl<1>({_SAMPLER})": [
        "test_gpu_parity::test_sampler_fast_path_vs_oracle", "test_gpu_parity::test_sampler_padding_modes_vs_torch",
        "test_gpu_sampler_referee::test_sampler_forward_on_decisions"],
    f"void enarf::sample_fwd_cl<2>({_SAMPLER})": [
        "test_gpu_parity::test_sampler_fast_path_vs_oracle", "test_gpu_parity::test_sampler_fast_path_channel_widths_at_tile_edges",
        "test_gpu_sampler_referee::test_sampler_forward_on_decisions"],
    f"void enarf::sample_fwd_cl<4>({_SAMPLER})": [
        "test_gpu_parity::test_sampler_fast_path_vs_oracle", "test_gpu_api::test_sampler_autograd_function_gives_true_gradients",
        "test_gpu_sampler_referee::test_sampler_forward_on_decisions"],
    f"void enarf::sample_fwd_cl<8>({_SAMPLER})": [
        "test_gpu_parity::test_sampler_fast_path_vs_oracle", "test_gpu_parity::test_sampler_fast_path_channel_widths_at_tile_edges",
        "test_gpu_sampler_referee::test_sampler_forward_on_decisions"],
    "void enarf::sample_fwd_direct<false>(float const*, float const*, float*, int, int, int, long long, enarf::SamplerCfg, int const*, int)": [
        "test_gpu_parity::test_sampler_fast_path_vs_oracle", "test_gpu_parity::test_sampler_padding_modes_vs_torch",
        "test_gpu_parity::test_sampler_golden_fwd_bwd",
        "test_gpu_sampler_referee::test_sampler_forward_on_decisions",
        "test_gpu_sampler_referee::test_sampler_nearest_rounds_half_away_from_zero",
        "test_gpu_sampler_referee::test_sampler_separate_planes_and_point_image"],
    "void enarf::sample_fwd_direct<true>(float const*, float const*, float*, int, int, int, long long, enarf::SamplerCfg, int const*, int)": [
        "test_gpu_api::test_sampler_image_ids_outside_the_batch_sample_nothing", "test_gpu_api::test_sampling_api_mirror_matches_reference_golden",
        "test_gpu_sampler_referee::test_sampler_separate_planes_and_point_image"],
    "enarf::sample_bwd_cl32(float const*, float const*, float const*, float*, float*, int, int, long long, enarf::SamplerCfg)": [
        "test_gpu_parity::test_sampler_backward_fast_path_vs_direct_and_autograd", "test_gpu_api::test_sampler_autograd_function_gives_true_gradients",
        "test_gpu_sampler_referee::test_sampler_backward_fast_path_on_decisions",
        "test_gpu_sampler_referee::test_sampler_backward_contention_on_one_footprint"],
    "enarf::sample_bwd_direct(float const*, float const*, float const*, float*, float*, int, int, int, long long, enarf::SamplerCfg, int, int const*, int)": [
        "test_gpu_parity::test_sampler_backward_fast_path_vs_direct_and_autograd", "test_gpu_parity::test_sampler_golden_fwd_bwd",
        "test_gpu_api::test_sampling_api_mirror_matches_reference_golden",
        "test_gpu_sampler_referee::test_sampler_backward_direct_on_decisions",
        "test_gpu_sampler_referee::test_sampler_nearest_rounds_half_away_from_zero",
        "test_gpu_sampler_referee::test_sampler_separate_planes_and_point_image",
        "test_gpu_sampler_referee::test_sampler_backward_contention_on_one_footprint"],
    "enarf::unpack_add_kernel(float const*, float*, int, int, int)": [
        "test_gpu_parity::test_sampler_backward_fast_path_vs_direct_and_autograd", "test_gpu_backward::test_render_backward_matches_oracle_autograd",
        "test_gpu_backward::test_query_backward_matches_oracle_autograd",
        "test_gpu_backward_f64::test_render_bwd_feature_gradient_channel_last",
        "test_gpu_sampler_referee::test_sampler_backward_fast_path_on_decisions",
        "test_gpu_sampler_referee::test_sampler_backward_contention_on_one_footprint"],
    "enarf::warp_fwd_kernel(float const*, float const*, float*, int, int)": [
        "test_gpu_parity::test_deformation_field_producer_vs_grid_sample", "test_gpu_backward::test_model_with_deformation_field_producer",
        "test_gpu_sampler_referee::test_warp_on_decisions_and_tails"],
    "enarf::warp_bwd_kernel(float const*, float const*, float const*, float*, float*, int, int)": [
        "test_gpu_parity::test_deformation_field_producer_vs_grid_sample", "test_gpu_backward::test_model_with_deformation_field_producer",
        "test_gpu_sampler_referee::test_warp_on_decisions_and_tails"],
    # ---- ray sampling (csrc/enarf_raysample.hip)
    "enarf::topk_select_kernel(float const*, long long*, int, int)": [
        "test_gpu_api::test_mask_based_sampler_matches_torch", "test_gpu_api::test_dso_generator_forward_matches_oracle_on_sampled_rays",
        "test_gpu_sampler_referee::test_ray_sampler_against_the_referee",
        "test_gpu_sampler_referee::test_ray_sampler_ties_take_the_lowest_flat_indices",
        "test_gpu_sampler_referee::test_ray_sampler_more_ties_than_the_buffer_holds"],
    "void enarf::window_max_kernel<false>(float const*, float*, int, int, int, float const*)": [
        "test_gpu_api::test_mask_based_sampler_matches_torch", "test_gpu_api::test_dso_generator_forward_matches_oracle_on_sampled_rays",
        "test_gpu_sampler_referee::test_ray_sampler_against_the_referee",
        "test_gpu_sampler_referee::test_ray_sampler_ties_take_the_lowest_flat_indices",
        "test_gpu_sampler_referee::test_ray_sampler_more_ties_than_the_buffer_holds"],
    "void enarf::window_max_kernel<true>(float const*, float*, int, int, int, float const*)": [
        "test_gpu_api::test_mask_based_sampler_matches_torch", "test_gpu_api::test_dso_generator_forward_matches_oracle_on_sampled_rays",
        "test_gpu_sampler_referee::test_ray_sampler_against_the_referee",
        "test_gpu_sampler_referee::test_ray_sampler_ties_take_the_lowest_flat_indices",
        "test_gpu_sampler_referee::test_ray_sampler_more_ties_than_the_buffer_holds"],
    # ---- renderer forward (csrc/enarf_render.hip); mode 0 f32, 1 bf16x3, 2 bf16, 3 f16x3; second argument samples per lane
    "enarf::prepare_kernel(enarf::PrepareParams)": [
        "test_gpu_parity::test_prepare_matches_oracle", "test_gpu_parity::test_render_vs_oracle_and_golden",
        "test_gpu_parity::test_query_vs_oracle_and_golden"],
    "enarf::mlp_unpack_kernel(float const*, float*)": ["test_gpu_parity::test_prepare_matches_oracle"],
    "void enarf::near_far_kernel<false>(float const*, enarf_prepare_args, int, int, float*)": [
        "test_gpu_configs::test_gan_batches_with_per_image_triplanes_at_128", "test_gpu_configs::test_grouped_batch_gives_the_same_bits_as_one_launch"],
    "void enarf::near_far_kernel<true>(float const*, enarf_prepare_args, int, int, float*)": [
        "test_gpu_configs::test_grouped_batch_gives_the_same_bits_as_one_launch"],
    "enarf::pre_march_kernel(enarf::PreParams)": [
        "test_gpu_parity::test_fused_step_is_bit_identical_to_separate_calls", "test_gpu_configs::test_grouped_batch_gives_the_same_bits_as_one_launch"],
    "enarf::ray_setup_kernel(enarf_render_args, int)": [
        "test_gpu_parity::test_render_vs_oracle_and_golden", "test_gpu_parity::test_render_sample_count_variants_vs_oracle"],
    f"void enarf::render_kernel<0, 1>({_RA})": [
        "test_gpu_parity::test_render_vs_oracle_and_golden", "test_gpu_parity::test_both_march_kernels_give_the_same_bits",
        "test_gpu_forward_f64::test_forward_march_vs_float64"],
    f"void enarf::render_kernel<0, 2>({_RA})": [
        "test_gpu_parity::test_render_vs_oracle_and_golden", "test_gpu_parity::test_both_march_kernels_give_the_same_bits",
        "test_gpu_forward_f64::test_forward_march_vs_float64"],
    f"void enarf::render_kernel<1, 1>({_RA})": ["test_gpu_parity::test_bf16_modes_both_march_kernels_vs_oracle",
        "test_gpu_forward_f64::test_forward_march_vs_float64"],
    f"void enarf::render_kernel<1, 2>({_RA})": ["test_gpu_parity::test_bf16_modes_both_march_kernels_vs_oracle",
        "test_gpu_forward_f64::test_forward_march_vs_float64"],
    f"void enarf::render_kernel<2, 1>({_RA})": ["test_gpu_parity::test_bf16_modes_both_march_kernels_vs_oracle",
        "test_gpu_forward_f64::test_forward_march_vs_float64"],
    f"void enarf::render_kernel<2, 2>({_RA})": [
        "test_gpu_parity::test_bf16_modes_both_march_kernels_vs_oracle", "test_gpu_configs::test_c4_256_nc72_nf96_bf16_early_termination",
        "test_gpu_forward_f64::test_forward_march_vs_float64"],
    f"void enarf::render_kernel<3, 1>({_RA})": [
        "test_gpu_parity::test_render_vs_oracle_and_golden", "test_gpu_parity::test_both_march_kernels_give_the_same_bits",
        "test_gpu_forward_f64::test_forward_march_vs_float64"],
    f"void enarf::render_kernel<3, 2>({_RA})": [
        "test_gpu_parity::test_render_vs_oracle_and_golden", "test_gpu_parity::test_both_march_kernels_give_the_same_bits",
        "test_gpu_forward_f64::test_forward_march_vs_float64"],
    f"void enarf::march_kernel<0, 1, 12>({_RA}, int, unsigned int*)": ["test_gpu_parity::test_both_march_kernels_give_the_same_bits",
        "test_gpu_forward_f64::test_forward_march_vs_float64"],
    f"void enarf::march_kernel<0, 2, 12>({_RA}, int, unsigned int*)": [
        "test_gpu_parity::test_both_march_kernels_give_the_same_bits", "test_gpu_parity::test_render_sample_count_variants_vs_oracle",
        "test_gpu_forward_f64::test_forward_march_vs_float64"],
    f"void enarf::march_kernel<1, 1, 12>({_RA}, int, unsigned int*)": ["test_gpu_parity::test_bf16_modes_both_march_kernels_vs_oracle",
        "test_gpu_forward_f64::test_forward_march_vs_float64"],
    f"void enarf::march_kernel<1, 2, 12>({_RA}, int, unsigned int*)": ["test_gpu_parity::test_bf16_modes_both_march_kernels_vs_oracle",
        "test_gpu_forward_f64::test_forward_march_vs_float64"],
    f"void enarf::march_kernel<2, 1, 12>({_RA}, int, unsigned int*)": ["test_gpu_parity::test_bf16_modes_both_march_kernels_vs_oracle",
        "test_gpu_forward_f64::test_forward_march_vs_float64"],
    f"void enarf::march_kernel<2, 2, 12>({_RA}, int, unsigned int*)": ["test_gpu_parity::test_bf16_modes_both_march_kernels_vs_oracle",
        "test_gpu_forward_f64::test_forward_march_vs_float64"],
    f"void enarf::march_kernel<3, 1, 12>({_RA}, int, unsigned int*)": ["test_gpu_parity::test_both_march_kernels_give_the_same_bits",
        "test_gpu_forward_f64::test_forward_march_vs_float64"],
    f"void enarf::march_kernel<3, 2, 12>({_RA}, int, unsigned int*)": ["test_gpu_parity::test_both_march_kernels_give_the_same_bits",
        "test_gpu_forward_f64::test_forward_march_vs_float64"],
    f"void enarf::query_kernel<0, false>({_QA})": [
        "test_gpu_parity::test_query_culling_does_not_depend_on_stale_lds", "test_gpu_parity::test_query_multiply_density_with_weight"],
    f"void enarf::query_kernel<0, true>({_QA})": [
        "test_gpu_parity::test_query_vs_oracle_and_golden", "test_gpu_parity::test_query_points_on_the_faces_of_the_canonical_cube",
        "test_gpu_forward_f64::test_query_fwd_placed_points_vs_float64"],
    f"void enarf::query_kernel<1, false>({_QA})": ["test_gpu_parity::test_query_debug_and_production_kernels_in_bf16_modes"],
    f"void enarf::query_kernel<1, true>({_QA})": [
        "test_gpu_parity::test_query_vs_oracle_and_golden", "test_gpu_parity::test_query_debug_and_production_kernels_in_bf16_modes",
        "test_gpu_forward_f64::test_query_fwd_placed_points_vs_float64"],
    f"void enarf::query_kernel<2, false>({_QA})": [
        "test_gpu_parity::test_query_bf16_mode_is_close", "test_gpu_parity::test_query_debug_and_production_kernels_in_bf16_modes"],
    f"void enarf::query_kernel<2, true>({_QA})": ["test_gpu_parity::test_query_debug_and_production_kernels_in_bf16_modes",
        "test_gpu_forward_f64::test_query_fwd_placed_points_vs_float64"],
    f"void enarf::query_kernel<3, false>({_QA})": [
        "test_gpu_api::test_gan_generator_forward_matches_oracle", "test_gpu_api::test_model_query_entry_point_matches_reference_golden"],
    f"void enarf::query_kernel<3, true>({_QA})": [
        "test_gpu_parity::test_query_vs_oracle_and_golden", "test_gpu_parity::test_query_points_on_the_faces_of_the_canonical_cube",
        "test_gpu_forward_f64::test_query_fwd_placed_points_vs_float64"],
    # ---- renderer backward (csrc/enarf_render_bwd.hip)
    "void enarf::render_bwd_kernel<1>(enarf_render_bwd_args)": [
        "test_gpu_backward::test_render_backward_matches_oracle_autograd", "test_gpu_backward::test_render_backward_matches_reference_gradients",
        "test_gpu_backward_f64::test_render_bwd_fine_counts_vs_float64", "test_gpu_backward_f64::test_render_bwd_parts_style_and_batch_vs_float64",
        "test_gpu_backward_f64::test_render_bwd_shared_triplane_three_images_vs_float64",
        "test_gpu_backward_f64::test_render_bwd_group_frames_vs_float64_and_each_other"],
    "void enarf::render_bwd_kernel<2>(enarf_render_bwd_args)": [
        "test_gpu_backward::test_render_backward_fine_counts_and_density_modes", "test_gpu_backward_sizes::test_backward_c4_shape_256_nf96",
        "test_gpu_backward_f64::test_render_bwd_fine_counts_vs_float64"],
    "enarf::query_bwd_kernel(enarf_query_bwd_args, long long)": [
        "test_gpu_backward::test_query_backward_matches_oracle_autograd", "test_gpu_backward::test_query_modes_forward_and_backward",
        "test_gpu_backward_f64::test_query_bwd_placed_points_vs_float64"],
    "enarf::weight_grad_partial_kernel(enarf::WeightGradParams)": [
        "test_gpu_backward::test_render_backward_matches_oracle_autograd", "test_gpu_backward::test_query_backward_matches_oracle_autograd",
        "test_gpu_backward_f64::test_weight_grad_vs_float64", "test_gpu_backward_f64::test_render_bwd_fine_counts_vs_float64"],
    "enarf::weight_grad_reduce_kernel(enarf::WeightGradParams)": [
        "test_gpu_backward::test_render_backward_matches_oracle_autograd", "test_gpu_backward::test_query_backward_matches_oracle_autograd",
        "test_gpu_backward_f64::test_weight_grad_vs_float64", "test_gpu_backward_f64::test_render_bwd_fine_counts_vs_float64"],
    "enarf::prepare_bwd_kernel(enarf_prepare_bwd_args)": [
        "test_gpu_backward::test_render_backward_matches_oracle_autograd", "test_gpu_backward::test_query_backward_matches_oracle_autograd",
        "test_gpu_backward_f64::test_prepare_bwd_vs_float64"],
}

# ---- libenarf_mesh.so
MESH_KERNEL_TESTS = {
    "(anonymous namespace)::mc_count_kernel(float const*, int, int, int, float, int*, int*, long long*, long long*, long long)": [
        "test_gpu_mesh::test_marching_cubes_matches_reference",
        "test_gpu_mesh::test_667_cube_counts_match_torch",
    ],
    "(anonymous namespace)::mc_scan_kernel(long long*, long long*, long long, long*, long long*)": [
        "test_gpu_mesh::test_marching_cubes_matches_reference",
        "test_gpu_mesh::test_667_cube_counts_match_torch",
    ],
    "(anonymous namespace)::mc_emit_kernel(float const*, int, int, int, float, int const*, int const*, long long const*, long long const*, long long const*, float*, long*)": [
        "test_gpu_mesh::test_marching_cubes_matches_reference",
        "test_gpu_mesh::test_closed_surfaces_are_watertight_and_deterministic",
        "test_gpu_mesh::test_667_cube_counts_match_torch",
    ],
}

# ---- libenarf_raster.so
_PROJ = "HIP_vector_type<double, 2u> const*, float const*"
RASTER_KERNEL_TESTS = {
    "(anonymous namespace)::raster_project_kernel(float const*, long long, float const*, double, HIP_vector_type<double, 2u>*, float*)": [
        "test_gpu_raster::test_hand_placed_triangles_match_reference",
        "test_gpu_raster::test_marching_cubes_meshes_match_reference",
    ],
    f"(anonymous namespace)::raster_depth_kernel(long const*, long long, long long, {_PROJ}, int, unsigned long long*, int*, int*)": [
        "test_gpu_raster::test_hand_placed_triangles_match_reference",
        "test_gpu_raster::test_marching_cubes_meshes_match_reference",
    ],
    f"(anonymous namespace)::raster_big_kernel(long const*, long long, {_PROJ}, int, unsigned long long*, int const*, int const*)": [
        "test_gpu_raster::test_hand_placed_triangles_match_reference",
        "test_gpu_raster::test_screen_filling_triangles_match_reference",
    ],
    "(anonymous namespace)::raster_mark_kernel(unsigned long long const*, long long, long const*, int*, int*, int*, long long)": [
        "test_gpu_raster::test_hand_placed_triangles_match_reference",
        "test_gpu_raster::test_marching_cubes_meshes_match_reference",
    ],
    "(anonymous namespace)::raster_count_kernel(long const*, long long, long long, int const*, int*)": [
        "test_gpu_raster::test_marching_cubes_meshes_match_reference",
    ],
    "(anonymous namespace)::raster_scan_kernel(int const*, int const*, long long, long long*)": [
        "test_gpu_raster::test_marching_cubes_meshes_match_reference",
    ],
    "(anonymous namespace)::raster_fill_kernel(long const*, long long, long long, int const*, int*, long long const*, int*)": [
        "test_gpu_raster::test_marching_cubes_meshes_match_reference",
    ],
    "(anonymous namespace)::raster_vnormal_kernel(float const*, long const*, int const*, long long, long long const*, int*, double*)": [
        "test_gpu_raster::test_marching_cubes_meshes_match_reference",
        "test_gpu_raster::test_hand_placed_triangles_match_reference",
    ],
    f"(anonymous namespace)::raster_shade_kernel(unsigned long long const*, int, long const*, long long, float const*, {_PROJ}, int const*, double const*, unsigned char*, long*, float*, float*, float*)": [
        "test_gpu_raster::test_hand_placed_triangles_match_reference",
        "test_gpu_raster::test_marching_cubes_meshes_match_reference",
        "test_gpu_raster::test_empty_mesh_is_all_background",
    ],
}

# ---- libenarf_pose.so
_POSE_ARGS = "(anonymous namespace)::Args"
POSE_KERNEL_TESTS = {
    f"void (anonymous namespace)::pose_mask_kernel<{d}, {k}>({_POSE_ARGS})": tests
    for (d, k), tests in {
        ("true", "true"): ["test_gpu_pose::test_kernel_matches_restatement_bit_for_bit",
                           "test_gpu_pose::test_edge_cases_match_restatement",
                           "test_gpu_pose::test_kernel_matches_reference_goldens"],
        ("true", "false"): ["test_gpu_pose::test_null_outputs_are_not_written"],
        ("false", "true"): ["test_gpu_pose::test_null_outputs_are_not_written"],
        ("false", "false"): ["test_gpu_pose::test_kernel_matches_restatement_bit_for_bit",
                             "test_gpu_pose::test_dataset_batches_reproduce_reference_items"],
    }.items()
}

# ---- libenarf_photo.so
_NS = "(anonymous namespace)::"
_LOSS_TESTS = ["test_gpu_photo::test_loss_matches_restatement", "test_gpu_photo::test_loss_matches_reference_fixture",
               "test_gpu_photo::test_two_runs_give_identical_bits"]
_METRIC_TESTS = ["test_gpu_photo::test_metrics_match_restatement", "test_gpu_photo::test_metrics_rectangles",
                 "test_gpu_photo::test_two_runs_give_identical_bits"]
PHOTO_KERNEL_TESTS = {
    f"{_NS}photo_loss_kernel({_NS}LossArgs, double*)": _LOSS_TESTS,
    f"{_NS}photo_loss_finish_kernel(double const*, int, double, double, double, double, int, float*)": _LOSS_TESTS,
    f"{_NS}photo_loss_bwd_kernel({_NS}LossArgs, float const*, float const*, float*, float*)": _LOSS_TESTS,
    f"{_NS}photo_metrics_kernel({_NS}MetricArgs, double*)": _METRIC_TESTS,
    f"{_NS}photo_metrics_finish_kernel({_NS}MetricArgs, double const*, float*)": _METRIC_TESTS,
}

# ---- libenarf_guide.so (guide_hist_kernel is launched only when the push term is on: each of its tests runs a ratio > 0)
_GUIDE_TESTS = ["test_gpu_mask_guidance::test_fixture_cases_match_reference_and_referee",
                "test_gpu_mask_guidance::test_training_sizes_match_referee_and_are_no_further_from_it_than_torch",
                "test_gpu_mask_guidance::test_two_runs_give_identical_bits"]
GUIDE_KERNEL_TESTS = {
    f"{_NS}guide_hist_kernel({_NS}Args, int, {_NS}Work*)": _GUIDE_TESTS,
    f"{_NS}guide_sum_kernel({_NS}Args, {_NS}Work*, int*)": _GUIDE_TESTS,
    f"{_NS}guide_finish_kernel({_NS}Args, int, {_NS}Work const*, int*, float*)": _GUIDE_TESTS,
    f"{_NS}guide_bwd_kernel({_NS}Args, int const*, float const*, float*)": _GUIDE_TESTS,
}

# one map per row of enarf_gan_amd.build.LIBRARIES, and the one GPU test module the side libraries' entries name
LIBRARY_KERNEL_TESTS = {"hip": KERNEL_TESTS, "mesh": MESH_KERNEL_TESTS, "raster": RASTER_KERNEL_TESTS, "pose": POSE_KERNEL_TESTS,
                        "photo": PHOTO_KERNEL_TESTS, "guide": GUIDE_KERNEL_TESTS}
GPU_TEST_MODULE = {"mesh": "test_gpu_mesh", "raster": "test_gpu_raster", "pose": "test_gpu_pose", "photo": "test_gpu_photo",
                   "guide": "test_gpu_mask_guidance"}
