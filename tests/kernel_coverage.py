"""Which GPU tests launch each kernel instantiation of libenarf_hip.so and compare its output with a reference.

Keys: every instantiation the library builds, demangled as its `.kd` (kernel descriptor) symbol prints
(tools/check_mfma_chains.kernel_symbols); values: `module::function` of tests under tests/. A kernel-trace run of the GPU
suite (rocprofv3 --kernel-trace) is what these entries were read from. tests/test_kernel_coverage_cpu.py requires the keys to
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
        "test_gpu_parity::test_sampler_fast_path_vs_oracle", "test_gpu_parity::test_sampler_padding_modes_vs_torch"],
    f"void enarf::pack_kernel<16>({_PACK})": [
        "test_gpu_parity::test_sampler_fast_path_vs_oracle", "test_gpu_parity::test_sampler_fast_path_channel_widths_at_tile_edges"],
    f"void enarf::pack_kernel<32>({_PACK})": [
        "test_gpu_parity::test_sampler_fast_path_vs_oracle", "test_gpu_parity::test_render_vs_oracle_and_golden",
        "test_gpu_parity::test_query_vs_oracle_and_golden"],
    f"void enarf::pack_kernel<64>({_PACK})": [
        "test_gpu_parity::test_sampler_fast_path_vs_oracle", "test_gpu_parity::test_sampler_fast_path_channel_widths_at_tile_edges"],
    f"void enarf::sample_fwd_cl<1>({_SAMPLER})": [
        "test_gpu_parity::test_sampler_fast_path_vs_oracle", "test_gpu_parity::test_sampler_padding_modes_vs_torch"],
    f"void enarf::sample_fwd_cl<2>({_SAMPLER})": [
        "test_gpu_parity::test_sampler_fast_path_vs_oracle", "test_gpu_parity::test_sampler_fast_path_channel_widths_at_tile_edges"],
    f"void enarf::sample_fwd_cl<4>({_SAMPLER})": [
        "test_gpu_parity::test_sampler_fast_path_vs_oracle", "test_gpu_api::test_sampler_autograd_function_gives_true_gradients"],
    f"void enarf::sample_fwd_cl<8>({_SAMPLER})": [
        "test_gpu_parity::test_sampler_fast_path_vs_oracle", "test_gpu_parity::test_sampler_fast_path_channel_widths_at_tile_edges"],
    "void enarf::sample_fwd_direct<false>(float const*, float const*, float*, int, int, int, long long, enarf::SamplerCfg, int const*, int)": [
        "test_gpu_parity::test_sampler_fast_path_vs_oracle", "test_gpu_parity::test_sampler_padding_modes_vs_torch",
        "test_gpu_parity::test_sampler_golden_fwd_bwd"],
    "void enarf::sample_fwd_direct<true>(float const*, float const*, float*, int, int, int, long long, enarf::SamplerCfg, int const*, int)": [
        "test_gpu_api::test_sampler_image_ids_outside_the_batch_sample_nothing", "test_gpu_api::test_sampling_api_mirror_matches_reference_golden"],
    "enarf::sample_bwd_cl32(float const*, float const*, float const*, float*, float*, int, int, long long, enarf::SamplerCfg)": [
        "test_gpu_parity::test_sampler_backward_fast_path_vs_direct_and_autograd", "test_gpu_api::test_sampler_autograd_function_gives_true_gradients"],
    "enarf::sample_bwd_direct(float const*, float const*, float const*, float*, float*, int, int, int, long long, enarf::SamplerCfg, int, int const*, int)": [
        "test_gpu_parity::test_sampler_backward_fast_path_vs_direct_and_autograd", "test_gpu_parity::test_sampler_golden_fwd_bwd",
        "test_gpu_api::test_sampling_api_mirror_matches_reference_golden"],
    "enarf::unpack_add_kernel(float const*, float*, int, int, int)": [
        "test_gpu_parity::test_sampler_backward_fast_path_vs_direct_and_autograd", "test_gpu_backward::test_render_backward_matches_oracle_autograd",
        "test_gpu_backward::test_query_backward_matches_oracle_autograd",
        "test_gpu_backward_f64::test_render_bwd_feature_gradient_channel_last"],
    "enarf::warp_fwd_kernel(float const*, float const*, float*, int, int)": [
        "test_gpu_parity::test_deformation_field_producer_vs_grid_sample", "test_gpu_backward::test_model_with_deformation_field_producer"],
    "enarf::warp_bwd_kernel(float const*, float const*, float const*, float*, float*, int, int)": [
        "test_gpu_parity::test_deformation_field_producer_vs_grid_sample", "test_gpu_backward::test_model_with_deformation_field_producer"],
    # ---- ray sampling (csrc/enarf_raysample.hip)
    "enarf::topk_select_kernel(float const*, long long*, int, int)": [
        "test_gpu_api::test_mask_based_sampler_matches_torch", "test_gpu_api::test_dso_generator_forward_matches_oracle_on_sampled_rays"],
    "void enarf::window_max_kernel<false>(float const*, float*, int, int, int, float const*)": [
        "test_gpu_api::test_mask_based_sampler_matches_torch", "test_gpu_api::test_dso_generator_forward_matches_oracle_on_sampled_rays"],
    "void enarf::window_max_kernel<true>(float const*, float*, int, int, int, float const*)": [
        "test_gpu_api::test_mask_based_sampler_matches_torch", "test_gpu_api::test_dso_generator_forward_matches_oracle_on_sampled_rays"],
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
        "test_gpu_parity::test_render_vs_oracle_and_golden", "test_gpu_parity::test_both_march_kernels_give_the_same_bits"],
    f"void enarf::render_kernel<0, 2>({_RA})": [
        "test_gpu_parity::test_render_vs_oracle_and_golden", "test_gpu_parity::test_both_march_kernels_give_the_same_bits"],
    f"void enarf::render_kernel<1, 1>({_RA})": ["test_gpu_parity::test_bf16_modes_both_march_kernels_vs_oracle"],
    f"void enarf::render_kernel<1, 2>({_RA})": ["test_gpu_parity::test_bf16_modes_both_march_kernels_vs_oracle"],
    f"void enarf::render_kernel<2, 1>({_RA})": ["test_gpu_parity::test_bf16_modes_both_march_kernels_vs_oracle"],
    f"void enarf::render_kernel<2, 2>({_RA})": [
        "test_gpu_parity::test_bf16_modes_both_march_kernels_vs_oracle", "test_gpu_configs::test_c4_256_nc72_nf96_bf16_early_termination"],
    f"void enarf::render_kernel<3, 1>({_RA})": [
        "test_gpu_parity::test_render_vs_oracle_and_golden", "test_gpu_parity::test_both_march_kernels_give_the_same_bits"],
    f"void enarf::render_kernel<3, 2>({_RA})": [
        "test_gpu_parity::test_render_vs_oracle_and_golden", "test_gpu_parity::test_both_march_kernels_give_the_same_bits"],
    f"void enarf::march_kernel<0, 1, 12>({_RA}, int, unsigned int*)": ["test_gpu_parity::test_both_march_kernels_give_the_same_bits"],
    f"void enarf::march_kernel<0, 2, 12>({_RA}, int, unsigned int*)": [
        "test_gpu_parity::test_both_march_kernels_give_the_same_bits", "test_gpu_parity::test_render_sample_count_variants_vs_oracle"],
    f"void enarf::march_kernel<1, 1, 12>({_RA}, int, unsigned int*)": ["test_gpu_parity::test_bf16_modes_both_march_kernels_vs_oracle"],
    f"void enarf::march_kernel<1, 2, 12>({_RA}, int, unsigned int*)": ["test_gpu_parity::test_bf16_modes_both_march_kernels_vs_oracle"],
    f"void enarf::march_kernel<2, 1, 12>({_RA}, int, unsigned int*)": ["test_gpu_parity::test_bf16_modes_both_march_kernels_vs_oracle"],
    f"void enarf::march_kernel<2, 2, 12>({_RA}, int, unsigned int*)": ["test_gpu_parity::test_bf16_modes_both_march_kernels_vs_oracle"],
    f"void enarf::march_kernel<3, 1, 12>({_RA}, int, unsigned int*)": ["test_gpu_parity::test_both_march_kernels_give_the_same_bits"],
    f"void enarf::march_kernel<3, 2, 12>({_RA}, int, unsigned int*)": ["test_gpu_parity::test_both_march_kernels_give_the_same_bits"],
    f"void enarf::query_kernel<0, false>({_QA})": [
        "test_gpu_parity::test_query_culling_does_not_depend_on_stale_lds", "test_gpu_parity::test_query_multiply_density_with_weight"],
    f"void enarf::query_kernel<0, true>({_QA})": [
        "test_gpu_parity::test_query_vs_oracle_and_golden", "test_gpu_parity::test_query_points_on_the_faces_of_the_canonical_cube"],
    f"void enarf::query_kernel<1, false>({_QA})": ["test_gpu_parity::test_query_debug_and_production_kernels_in_bf16_modes"],
    f"void enarf::query_kernel<1, true>({_QA})": [
        "test_gpu_parity::test_query_vs_oracle_and_golden", "test_gpu_parity::test_query_debug_and_production_kernels_in_bf16_modes"],
    f"void enarf::query_kernel<2, false>({_QA})": [
        "test_gpu_parity::test_query_bf16_mode_is_close", "test_gpu_parity::test_query_debug_and_production_kernels_in_bf16_modes"],
    f"void enarf::query_kernel<2, true>({_QA})": ["test_gpu_parity::test_query_debug_and_production_kernels_in_bf16_modes"],
    f"void enarf::query_kernel<3, false>({_QA})": [
        "test_gpu_api::test_gan_generator_forward_matches_oracle", "test_gpu_api::test_model_query_entry_point_matches_reference_golden"],
    f"void enarf::query_kernel<3, true>({_QA})": [
        "test_gpu_parity::test_query_vs_oracle_and_golden", "test_gpu_parity::test_query_points_on_the_faces_of_the_canonical_cube"],
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
