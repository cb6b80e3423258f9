#!/bin/sh
# Compare the device assembly of every csrc/*.hip of the working tree with that of a git revision.
# usage: tools/isa_compare.sh <git-rev> [kernel-regex]      (from anywhere inside the repository)
# Both trees are compiled with the Makefile's HIPFLAGS plus --cuda-device-only -S; the only text
# that differs between two builds of one source, the random __hip_cuid_<hex> symbol, is replaced
# by a fixed word.  Prints `identical` or the first differing lines per file; exits non-zero on
# any difference.  Takes a few minutes (one build of deflate_kernels.hip is ~45 s).
# With a kernel-regex (an extended regular expression on the demangled name, e.g.
# 'k_deflate_emit<[0-9]+, (true|false), false>|k_compact\(') the comparison is per function
# instead: the body from the function's label to its .Lfunc_end, for every function of either
# side whose name matches -- for a file that differs as a whole because other kernels in it
# changed.  The numbers the assembler gives a function by its position in the file (.LBB<k>_,
# .Lfunc_end<k>, and the BB<k>_ of the loop comments) are replaced by fixed words.
set -eu
[ $# -eq 1 ] || [ $# -eq 2 ] || { echo "usage: $0 <git-rev> [kernel-regex]" >&2; exit 2; }
filter=${2:-}
root=$(git rev-parse --show-toplevel)
tmp=$(mktemp -d)
trap 'rm -rf "$tmp"' EXIT
mkdir "$tmp/old" "$tmp/asm_old" "$tmp/asm_new"
git -C "$root" archive "$1" deflate.hpp_amd include | tar -x -C "$tmp/old"
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
CXXFILT=${CXXFILT:-c++filt}
flags=$(sed -n 's/^HIPFLAGS := //p' "$root/deflate.hpp_amd/Makefile")

# one line per compile job: <source> <output>
for side in old new; do
    [ $side = old ] && src=$tmp/old || src=$root
    for f in "$src"/deflate.hpp_amd/csrc/*.hip; do
        echo "$f $tmp/asm_$side/$(basename "$f" .hip).s"
    done
done | xargs -P 16 -L 1 sh -c "$HIPCC $flags --cuda-device-only -S \"\$0\" -o \"\$1\" 2>\"\$1.log\" || { cat \"\$1.log\" >&2; exit 255; }"

# the body of function $2 in assembly file $1, position-dependent label numbers removed
body() {
    awk -v f="$2:" 'index($0, f) == 1 { on = 1 } on { print } on && /^\.Lfunc_end[0-9]+:/ { exit }' "$1" |
        sed -E 's/\.LBB[0-9]+_/.LBB_/g; s/(Header=|Loop )BB[0-9]+_/\1BB_/g; s/^(\.LBB_[0-9]+:)[[:space:]]+;/\1 ;/; s/\.Lfunc_end[0-9]+/.Lfunc_end/g; s/__hip_cuid_[0-9a-f]+/__hip_cuid_X/g'
}

rc=0
for s in $(cd "$tmp" && ls asm_old asm_new | grep '\.s$' | sort -u); do
    for side in old new; do
        if [ -f "$tmp/asm_$side/$s" ]; then
            sed -E 's/__hip_cuid_[0-9a-f]+/__hip_cuid_X/g' "$tmp/asm_$side/$s" > "$tmp/$side.s"
        else
            : > "$tmp/$side.s"
        fi
    done
    if [ -n "$filter" ]; then
        # the functions of either side (label lines behind a .type ...,@function) that match
        cat "$tmp/old.s" "$tmp/new.s" | sed -n -E 's/^[[:space:]]*\.type[[:space:]]+([A-Za-z0-9_.$]+),@function.*/\1/p' |
            sort -u > "$tmp/syms"
        "$CXXFILT" < "$tmp/syms" | paste "$tmp/syms" - | grep -E "$(printf '\t').*($filter)" > "$tmp/match" || true
        while IFS="$(printf '\t')" read -r sym name; do
            body "$tmp/old.s" "$sym" > "$tmp/old.f"
            body "$tmp/new.s" "$sym" > "$tmp/new.f"
            if [ ! -s "$tmp/old.f" ] || [ ! -s "$tmp/new.f" ]; then
                [ -s "$tmp/old.f" ] && echo "${s%.s}.hip: $name: only in $1" || echo "${s%.s}.hip: $name: only in the working tree"
            elif cmp -s "$tmp/old.f" "$tmp/new.f"; then
                echo "${s%.s}.hip: $name: identical"
            else
                echo "${s%.s}.hip: $name: DIFFERS"
                diff "$tmp/old.f" "$tmp/new.f" | head -n 20
                rc=1
            fi
        done < "$tmp/match"
        continue
    fi
    if cmp -s "$tmp/old.s" "$tmp/new.s"; then
        echo "${s%.s}.hip: identical"
    else
        echo "${s%.s}.hip: DIFFERS"
        diff "$tmp/old.s" "$tmp/new.s" | head -n 20
        rc=1
    fi
done
exit $rc
