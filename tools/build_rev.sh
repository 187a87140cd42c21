#!/bin/bash
# Build libuvhttp_ws_amd.so from git revision REV into tools/bin/libws_REV.so (for
# tools/ab_lib.py A/B runs against the working tree's build).  Run here; the .so travels.
# The revision is exported whole and built by its own Makefile, so its sources, flags and
# object list are that revision's, whatever they were.
set -euo pipefail
ROOT=$(cd "$(dirname "$0")/.." && pwd)
REV=${1:?usage: build_rev.sh REV}
LIB=uvhttp_amd/lib/libuvhttp_ws_amd.so
TMP=$(mktemp -d)
trap 'rm -rf "$TMP"' EXIT
git -C "$ROOT" archive "$REV" | tar -x -C "$TMP"
make -C "$TMP" -j"${MAX_JOBS:-8}" "$LIB"
mkdir -p "$ROOT/tools/bin"
cp "$TMP/$LIB" "$ROOT/tools/bin/libws_$REV.so"
echo "$ROOT/tools/bin/libws_$REV.so"
