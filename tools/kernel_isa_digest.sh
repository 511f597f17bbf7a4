#!/bin/bash
# One line per object of a build directory: name, number of kernels, sha256 of the gfx950 disassembly, sha256 of the code
# object's notes (kernel names, register counts, spills, LDS, scratch).  Two builds emit the same device code exactly when
# their outputs are equal; host code is not covered.
# --kernels: one line per kernel symbol instead (object, sha256 of that symbol's instructions without addresses and
# encodings, mangled name), for objects whose set of kernels differs between two builds.
# usage: tools/kernel_isa_digest.sh [--kernels] lrp-imagecaptioning-pytorch_amd/csrc/build [object.o ...] > digest.txt
set -euo pipefail
per_kernel=0
if [ "${1:-}" = "--kernels" ]; then per_kernel=1; shift; fi
dir=${1:?usage: kernel_isa_digest.sh [--kernels] <build dir> [object.o ...]}
shift
bin=${ROCM_LLVM_BIN:-/opt/rocm/llvm/bin}
target=hipv4-amdgcn-amd-amdhsa--gfx950
tmp=$(mktemp -d)
trap 'rm -rf "$tmp"' EXIT
if [ $# -gt 0 ]; then objs=("$@"); else objs=($(cd "$dir" && ls *.o | sort)); fi
for o in "${objs[@]}"; do
  "$bin/llvm-objcopy" --dump-section .hip_fatbin="$tmp/x.fb" "$dir/$o" 2>/dev/null || { printf '%-24s (no device code)\n' "$o"; continue; }
  "$bin/clang-offload-bundler" --type=o --targets=$target --input="$tmp/x.fb" --output="$tmp/x.co" --unbundle
  "$bin/llvm-readelf" --notes "$tmp/x.co" > "$tmp/notes.txt"
  if [ $per_kernel = 1 ]; then
    # kernels = the symbols that have a descriptor (NAME.kd); a symbol's text runs to the next symbol header
    grep -o '[A-Za-z_][A-Za-z0-9_]*\.kd$' "$tmp/notes.txt" | sed 's/\.kd$//' | sort -u > "$tmp/kernels.txt"
    # (blank lines and the "..." of zero fill between symbols depend on what follows a kernel in its object, not on the kernel)
    "$bin/llvm-objdump" -d --no-leading-addr --no-show-raw-insn "$tmp/x.co" | sed 's,[[:space:]]*//.*$,,' | grep -v '^[[:space:]]*\(\.\.\.\)\?$' > "$tmp/dis.txt"
    # (nor does the run of s_nop / s_code_end padding behind a section's last kernel belong to that kernel: which kernel is last depends on the object)
    while read -r k; do
      h=$(awk -v s="<$k>:" '$NF == s { on = 1; next } /^[0-9a-f]* *<.*>:$/ { on = 0 } on { a[++n] = $0 }
                            END { while (n > 0 && a[n] ~ /^[[:space:]]*(s_nop 0|s_code_end)$/) --n; for (i = 1; i <= n; ++i) print a[i] }' "$tmp/dis.txt" | sha256sum | cut -c1-16)
      printf '%-24s %s %s\n' "$o" "$h" "$k"
    done < "$tmp/kernels.txt"
    continue
  fi
  # (the text, not the raw code object: comments in a header move line tables, not instructions)
  isa=$("$bin/llvm-objdump" -d "$tmp/x.co" | grep -v 'file format' | sha256sum | cut -c1-16)
  notes=$(sha256sum < "$tmp/notes.txt" | cut -c1-16)
  nk=$(grep -c '\.kd$' "$tmp/notes.txt" || true)
  printf '%-24s kernels %-4s isa %s notes %s\n' "$o" "$nk" "$isa" "$notes"
done
