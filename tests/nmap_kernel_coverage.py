"""Kernel -> GPU tests map of libenarf_nmap.so (the row `nmap` of enarf_gan_amd.build.LATE_LIBRARIES): every kernel the
library builds (demangled as its `.kd` symbol prints), each with the tests of tests/test_gpu_nmap.py that hold it to the float64 restatement of its contract
(tests/nmap_reference.py). tests/test_nmap_cpu.py checks the map against the built library and the test file."""
GPU_TEST_MODULE = "test_gpu_nmap"

_NS = "(anonymous namespace)::"
NMAP_KERNEL_TESTS = {
    f"{_NS}nmap_encode_kernel(enarf_nmap_encode_args)": [
        "test_gpu_nmap::test_encode_matches_the_referee_on_every_texel",
        "test_gpu_nmap::test_encode_bands_stitch_count_zero_and_two_runs_agree",
        "test_gpu_nmap::test_bake_normal_map_is_its_launches_by_hand"],
    f"{_NS}nmap_shade_kernel(enarf_nmap_shade_args, {_NS}Layout)": [
        "test_gpu_nmap::test_hand_written_fragments_match_the_referee",
        "test_gpu_nmap::test_unlit_normal_mapped_shade_equals_shade_textured_bit_for_bit",
        "test_gpu_nmap::test_the_normal_mapped_sphere_matches_the_referee",
        "test_gpu_nmap::test_a_constant_field_round_trips_on_the_device",
        "test_gpu_nmap::test_a_flat_map_gives_the_face_normal"],
}
