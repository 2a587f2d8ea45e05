"""What the CPU checks of the HIP libraries share: the rows of enarf_gan_amd.build.LIBRARIES, built once, with each row's
public header, binding module and kernel inventory (tests/test_libraries_cpu.py runs the generic checks over every row;
the test_*_cpu.py files keep what is specific to one library)."""
import functools
import importlib
import importlib.util
import os
import re

from enarf_gan_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTS = os.path.join(ROOT, "tests")
STEMS = list(build.LIBRARIES)


@functools.lru_cache(maxsize=None)
def tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@functools.lru_cache(maxsize=None)
def _build():
    return build.build()          # incremental: builds what this checkout has not yet


def library(stem):
    """path of the row's built library"""
    _build()
    return build.lib_path(stem)


def header(stem):
    return os.path.join(ROOT, "include", build.ALL_LIBRARIES[stem][1])      # rows of either table


def binding(stem):
    return importlib.import_module(build.binding(stem))


def prefix(stem):
    return "enarf_" if stem == "hip" else f"enarf_{stem}_"


def declared(stem):
    """every function the row's public header declares"""
    src = re.sub(r"/\*.*?\*/", "", open(header(stem)).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(%s[a-z0-9_]+)\s*\(" % prefix(stem), src)))


@functools.lru_cache(maxsize=None)
def kernels(stem):
    """kernel symbols of the row's built library"""
    return frozenset(tool("check_mfma_chains").kernel_symbols(library(stem)))
