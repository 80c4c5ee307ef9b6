#!/bin/bash
# Machine-code comparison of two builds of libics_hip.so (or of two gfx950 code objects), kernel by kernel:
#   scripts/isa_diff.sh OLD.so NEW.so
# Both files are unpacked like scripts/isa_table.sh does, every kernel is disassembled on its own, and addresses, encodings, branch
# targets and literal symbol addresses are stripped.  Output: per kernel `identical` or the number of differing lines (`only in OLD` /
# `only in NEW` for a kernel one side lacks), then a summary and both register tables (identical tables print once).  Exit status 1 when
# anything differs.  Compares two builds with each other and nothing else; needs no GPU.
set -e
[ $# -eq 2 ] || { echo "usage: $0 OLD.so NEW.so" >&2; exit 2; }
LLVM=/opt/rocm/lib/llvm/bin
HERE=$(cd "$(dirname "$0")" && pwd)
T=$(mktemp -d)
trap 'rm -rf $T' EXIT
unpack() {   # $1 = file, $2 = directory that receives one normalised listing per kernel
  mkdir -p $2
  cp "$1" $2/in.bin
  ( cd $2
    if head -c 24 in.bin | grep -q "__CLANG_OFFLOAD_BUNDLE__"; then
      $LLVM/clang-offload-bundler --unbundle --type=o --input=in.bin --targets=hipv4-amdgcn-amd-amdhsa--gfx950 --output=x.gfx950
    elif $LLVM/llvm-readelf -h in.bin 2>/dev/null | grep -q "AMDGPU"; then cp in.bin x.gfx950
    else $LLVM/llvm-objdump --offloading in.bin > /dev/null; fi
    # one listing per function symbol (mangled name): the `// ADDRESS: ENCODING <symbol+offset>` tails, branch targets and the
    # literals of pc-relative symbol arithmetic (s_getpc_b64 + s_add_u32 / s_addc_u32) go
    for f in *gfx950; do $LLVM/llvm-objdump -d --no-show-raw-insn "$f"; done |
      awk '/^[0-9a-f]+ <.*>:$/ { out = "k/" substr($2, 2, length($2) - 3); next }
           out != "" && /^\t/ { sub(/[ \t]*\/\/ [0-9A-F]+:.*$/, "")
                                if ($1 ~ /^s_(cbranch|branch|call)/) $0 = "\t" $1 " <target>"
                                if ($1 ~ /^s_addc?_u32$/ && $NF ~ /^0x/) { $NF = "<literal>"; $0 = "\t" $0 }
                                print >> out; close(out) }'
  )
}
mkdir -p $T/a/k $T/b/k
unpack "$1" $T/a
unpack "$2" $T/b
same=0; diffs=0
for n in $( (ls $T/a/k; ls $T/b/k) | sort -u ); do
  d=$(echo "$n" | c++filt | sed 's/(anonymous namespace):://g; s/^void //; s/(.*//')
  if [ ! -f $T/a/k/$n ]; then echo "$d: only in NEW"; diffs=$((diffs + 1))
  elif [ ! -f $T/b/k/$n ]; then echo "$d: only in OLD"; diffs=$((diffs + 1))
  elif cmp -s $T/a/k/$n $T/b/k/$n; then echo "$d: identical"; same=$((same + 1))
  else echo "$d: $(diff $T/a/k/$n $T/b/k/$n | grep -c '^[<>]') lines differ"; diffs=$((diffs + 1)); fi
done
echo "== $same identical, $diffs different"
"$HERE/isa_table.sh" "$1" > $T/ta
"$HERE/isa_table.sh" "$2" > $T/tb
if cmp -s $T/ta $T/tb; then echo "== register tables: equal"; cat $T/ta
else echo "== register tables differ"; echo "-- OLD"; cat $T/ta; echo "-- NEW"; cat $T/tb; diffs=$((diffs + 1)); fi
[ $diffs -eq 0 ]
