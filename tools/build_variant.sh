#!/bin/bash
# tools/build_variant.sh NAME [-DFLAG=V ...]: a second build of the same ABI under variants/libenarf_NAME.so
# (git-ignored; used through bench.py --allow-variant --variant PATH / ENARF_VARIANT=NAME of the tools for A/B runs). The tuning
# values are constexprs in the sources: run this script of a copy of the tree in which one of them is edited.
# The sources and the flags are enarf_gan_amd.build's: this is its --variant mode.
set -e
cd "$(dirname "$0")/.."
python3 -m enarf_gan_amd.build --variant "$@"
