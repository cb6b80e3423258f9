#!/bin/sh
# Compare the device assembly of every csrc/*.hip of the working tree with that of a git revision.
# usage: tools/isa_compare.sh <git-rev>      (from anywhere inside the repository)
# Both trees are compiled with the Makefile's HIPFLAGS plus --cuda-device-only -S; the only text
# that differs between two builds of one source, the random __hip_cuid_<hex> symbol, is replaced
# by a fixed word.  Prints `identical` or the first differing lines per file; exits non-zero on
# any difference.  Takes a few minutes (one build of deflate_kernels.hip is ~45 s).
set -eu
[ $# -eq 1 ] || { echo "usage: $0 <git-rev>" >&2; exit 2; }
root=$(git rev-parse --show-toplevel)
tmp=$(mktemp -d)
trap 'rm -rf "$tmp"' EXIT
mkdir "$tmp/old" "$tmp/asm_old" "$tmp/asm_new"
git -C "$root" archive "$1" deflate.hpp_amd include | tar -x -C "$tmp/old"
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
flags=$(sed -n 's/^HIPFLAGS := //p' "$root/deflate.hpp_amd/Makefile")

# one line per compile job: <source> <output>
for side in old new; do
    [ $side = old ] && src=$tmp/old || src=$root
    for f in "$src"/deflate.hpp_amd/csrc/*.hip; do
        echo "$f $tmp/asm_$side/$(basename "$f" .hip).s"
    done
done | xargs -P 16 -L 1 sh -c "$HIPCC $flags --cuda-device-only -S \"\$0\" -o \"\$1\" 2>\"\$1.log\" || { cat \"\$1.log\" >&2; exit 255; }"

rc=0
for s in $(cd "$tmp" && ls asm_old asm_new | grep '\.s$' | sort -u); do
    for side in old new; do
        if [ -f "$tmp/asm_$side/$s" ]; then
            sed -E 's/__hip_cuid_[0-9a-f]+/__hip_cuid_X/g' "$tmp/asm_$side/$s" > "$tmp/$side.s"
        else
            : > "$tmp/$side.s"
        fi
    done
    if cmp -s "$tmp/old.s" "$tmp/new.s"; then
        echo "${s%.s}.hip: identical"
    else
        echo "${s%.s}.hip: DIFFERS"
        diff "$tmp/old.s" "$tmp/new.s" | head -n 20
        rc=1
    fi
done
exit $rc
