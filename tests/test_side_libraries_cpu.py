"""CPU checks of the rows of enarf_gan_amd.build.SIDE_LIBRARIES, one case per row: what tests/test_libraries_cpu.py checks
for each row of build.LIBRARIES (public header against the exported symbols and the binding's SIGNATURES, the ABI version,
the kernel inventory against the row's kernel -> GPU tests map, the headers the build tracks) and that no kernel of a side
library is part of any other library, main table or side table. A side library's registry is the module
tests/<stem>_kernel_coverage.py with <STEM>_KERNEL_TESTS and GPU_TEST_MODULE."""
import ast
import ctypes as C
import importlib
import itertools
import os
import re

import pytest

import libraries as L
from enarf_gan_amd import build

SIDE = list(build.SIDE_LIBRARIES)


def _header(stem):
    return os.path.join(L.ROOT, "include", build.SIDE_LIBRARIES[stem][1])


def _declared(stem):
    src = re.sub(r"/\*.*?\*/", "", open(_header(stem)).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(enarf_%s_[a-z0-9_]+)\s*\(" % stem, src)))


def test_the_two_tables_are_disjoint_and_build_walks_both():
    assert SIDE and not set(build.SIDE_LIBRARIES) & set(build.LIBRARIES)
    assert list(build.ALL_LIBRARIES) == list(build.LIBRARIES) + SIDE
    L.library("hip")                                      # build() makes every row of both tables
    for stem in SIDE:
        assert os.path.exists(build.lib_path(stem)) and build.binding(stem) == f"enarf_gan_amd._{stem}_lib"


@pytest.mark.parametrize("stem", SIDE)
def test_header_symbols_exported_and_bound_and_abi_version(stem):
    lib = C.CDLL(L.library(stem))
    mod = importlib.import_module(build.binding(stem))
    declared = _declared(stem)
    assert declared and set(mod.SIGNATURES) == set(declared)
    for fn in declared:
        assert hasattr(lib, fn), f"{fn} declared in {os.path.basename(_header(stem))} but not exported"
    assert getattr(mod.load(), f"enarf_{stem}_abi_version")() == mod.ABI_VERSION
    assert re.search(rf"#define\s+ENARF_{stem.upper()}_ABI_VERSION\s+{mod.ABI_VERSION}\s", open(_header(stem)).read())


@pytest.mark.parametrize("stem", SIDE)
def test_kernels_equal_the_registry_and_each_has_gpu_tests(stem):
    registry = importlib.import_module(f"{stem}_kernel_coverage")
    kernel_tests, module = getattr(registry, f"{stem.upper()}_KERNEL_TESTS"), registry.GPU_TEST_MODULE
    built = L.kernels(stem)
    assert not built - set(kernel_tests), f"kernels with no test named in the registry: {sorted(built - set(kernel_tests))}"
    assert not set(kernel_tests) - built, f"entries of the registry the library does not build: {sorted(set(kernel_tests) - built)}"
    tree = ast.parse(open(os.path.join(L.TESTS, module + ".py")).read())
    functions = {n.name for n in tree.body if isinstance(n, ast.FunctionDef)}
    for kernel, tests in kernel_tests.items():
        assert tests, f"{kernel}: no test"
        for t in tests:
            assert t.split("::")[0] == module and t.split("::")[1] in functions, f"{kernel}: {t} does not exist in {module}"


@pytest.mark.parametrize("stem", SIDE)
def test_build_tracks_every_included_header(stem):
    tracked = {os.path.basename(h) for h in build.lib_deps(stem)}
    seen, todo = set(), list(build.SIDE_LIBRARIES[stem][0])
    while todo:
        f = todo.pop()
        path = os.path.join(build.CSRC, f) if os.path.exists(os.path.join(build.CSRC, f)) else os.path.join(L.ROOT, "include", f)
        for inc in re.findall(r'#include\s+"([^"]+)"', open(path).read()):
            if inc not in seen:
                seen.add(inc)
                todo.append(inc)
    assert seen and seen <= tracked, seen - tracked


def test_no_kernel_of_a_side_library_is_in_another_library():
    for a, b in itertools.chain(itertools.product(SIDE, L.STEMS), itertools.combinations(SIDE, 2)):
        assert L.kernels(a) and not L.kernels(a) & L.kernels(b), f"a kernel of {build.lib_path(a)} inside {build.lib_path(b)}"
