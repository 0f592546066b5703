#!/bin/bash
# sha256 of the device assembly build.sh keeps (build/*-hip-amdgcn-amd-amdhsa-gfx950.s), normalised so that two builds
# with the same kernels hash alike: comments (block names differ with the host code around the kernels) and blank lines
# dropped, the compilation unit's id replaced by a constant.  A host-only change leaves every hash as it was.
#   tools/device_code_hash.sh [build directory, default: build]
set -e
dir="${1:-$(dirname "$0")/../build}"
for unit in rtx_api rtx_sort; do
	f="$dir/$unit-hip-amdgcn-amd-amdhsa-gfx950.s"
	[ -f "$f" ] || { echo "$f is missing: run ./build.sh first" >&2; exit 1; }
	h=$(sed -e 's/[ \t]*;.*$//' -e 's/__hip_cuid_[0-9a-f]*/__hip_cuid_X/g' "$f" | grep -v '^\s*$' | sha256sum | cut -d' ' -f1)
	echo "$unit $h"
done
