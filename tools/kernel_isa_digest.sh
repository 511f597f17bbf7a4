#!/bin/bash
# One line per object of a build directory: name, number of kernels, sha256 of the gfx950 disassembly, sha256 of the code
# object's notes (kernel names, register counts, spills, LDS, scratch).  Two builds emit the same device code exactly when
# their outputs are equal; host code is not covered.
# usage: tools/kernel_isa_digest.sh lrp-imagecaptioning-pytorch_amd/csrc/build [object.o ...] > digest.txt
set -euo pipefail
dir=${1:?usage: kernel_isa_digest.sh <build dir> [object.o ...]}
shift
bin=${ROCM_LLVM_BIN:-/opt/rocm/llvm/bin}
target=hipv4-amdgcn-amd-amdhsa--gfx950
tmp=$(mktemp -d)
trap 'rm -rf "$tmp"' EXIT
if [ $# -gt 0 ]; then objs=("$@"); else objs=($(cd "$dir" && ls *.o | sort)); fi
for o in "${objs[@]}"; do
  "$bin/llvm-objcopy" --dump-section .hip_fatbin="$tmp/x.fb" "$dir/$o" 2>/dev/null || { printf '%-24s (no device code)\n' "$o"; continue; }
  "$bin/clang-offload-bundler" --type=o --targets=$target --input="$tmp/x.fb" --output="$tmp/x.co" --unbundle
  # (the text, not the raw code object: comments in a header move line tables, not instructions)
  isa=$("$bin/llvm-objdump" -d "$tmp/x.co" | grep -v 'file format' | sha256sum | cut -c1-16)
  "$bin/llvm-readelf" --notes "$tmp/x.co" > "$tmp/notes.txt"
  notes=$(sha256sum < "$tmp/notes.txt" | cut -c1-16)
  nk=$(grep -c '\.kd$' "$tmp/notes.txt" || true)
  printf '%-24s kernels %-4s isa %s notes %s\n' "$o" "$nk" "$isa" "$notes"
done
