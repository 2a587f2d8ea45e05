"""CPU checks every HIP library gets, one case per row of enarf_gan_amd.build.LIBRARIES: the public header against the
exported symbols and the binding's SIGNATURES, the ABI version, the kernel inventory against the row's kernel -> GPU
tests map (tests/kernel_coverage.py), the headers the build tracks, and that no kernel is in two libraries."""
import ast
import ctypes as C
import itertools
import os
import re

import pytest

import libraries as L
from enarf_gan_amd import build
from kernel_coverage import GPU_TEST_MODULE, LIBRARY_KERNEL_TESTS


@pytest.mark.parametrize("stem", L.STEMS)
def test_header_symbols_exported_and_bound(stem):
    lib = C.CDLL(L.library(stem))
    signatures = L.binding(stem).SIGNATURES
    declared = L.declared(stem)
    assert declared
    name = os.path.basename(L.header(stem))
    for fn in declared:
        assert hasattr(lib, fn), f"{fn} declared in {name} but not exported by {os.path.basename(L.library(stem))}"
        assert fn in signatures, f"{fn} has no ctypes signature in {build.binding(stem)}"
    assert set(signatures) == set(declared)


@pytest.mark.parametrize("stem", L.STEMS)
def test_abi_version_of_header_library_and_binding(stem):
    L.library(stem)
    mod = L.binding(stem)
    assert getattr(mod.load(), L.prefix(stem) + "abi_version")() == mod.ABI_VERSION
    macro = "ENARF_ABI_VERSION" if stem == "hip" else f"ENARF_{stem.upper()}_ABI_VERSION"
    assert re.search(rf"#define\s+{macro}\s+{mod.ABI_VERSION}\s", open(L.header(stem)).read())


@pytest.mark.parametrize("stem", L.STEMS)
def test_kernels_equal_the_map_and_each_has_gpu_tests(stem):
    assert set(LIBRARY_KERNEL_TESTS) == set(L.STEMS)
    kernel_tests = LIBRARY_KERNEL_TESTS[stem]
    built = L.kernels(stem)
    assert not built - set(kernel_tests), f"instantiations with no test named in tests/kernel_coverage.py: {sorted(built - set(kernel_tests))}"
    assert not set(kernel_tests) - built, f"entries of tests/kernel_coverage.py the library does not build: {sorted(set(kernel_tests) - built)}"
    functions = {}
    for kernel, tests in kernel_tests.items():
        assert tests, f"{kernel}: no test"
        for t in tests:
            module, func = t.split("::")
            assert module == GPU_TEST_MODULE.get(stem, module), f"{kernel}: {t} is not in {GPU_TEST_MODULE[stem]}"
            if module not in functions:
                tree = ast.parse(open(os.path.join(L.TESTS, module + ".py")).read())
                functions[module] = {n.name for n in tree.body if isinstance(n, ast.FunctionDef)}
            assert func in functions[module], f"{kernel}: {t} does not exist"


@pytest.mark.parametrize("stem", L.STEMS)
def test_build_tracks_every_included_header(stem):
    """enarf_gan_amd.build rebuilds an object when any header its source includes (directly or through another header)
    changed: a header missing from the dependency list leaves the library stale after a header-only edit."""
    tracked = {os.path.basename(h) for h in build.lib_deps(stem)}
    seen, todo = set(), list(build.LIBRARIES[stem][0])
    while todo:
        f = todo.pop()
        path = os.path.join(build.CSRC, f) if os.path.exists(os.path.join(build.CSRC, f)) else os.path.join(L.ROOT, "include", f)
        for inc in re.findall(r'#include\s+"([^"]+)"', open(path).read()):
            if inc not in seen:
                seen.add(inc)
                todo.append(inc)
    assert seen and seen <= tracked, seen - tracked


def test_no_kernel_is_in_two_libraries():
    assert len(L.STEMS) >= 6
    for a, b in itertools.combinations(L.STEMS, 2):
        assert L.kernels(a) and L.kernels(b)
        assert not L.kernels(a) & L.kernels(b), f"a kernel of {build.lib_path(a)} inside {build.lib_path(b)}"
