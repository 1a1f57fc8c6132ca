#!/bin/bash
# Device code of two builds, kernel by kernel: unbundles the gfx950 code object of every .hip unit's .o in two csrc directories,
# disassembles both and compares the text.  Needs no GPU.  A missing object or a failed extraction is an error, not "identical".
#   tools/device_code_ab.sh PARENT/pointreggpt_amd/csrc NEW/pointreggpt_amd/csrc [unit ...]      (units: names without .hip; default all)
# A unit whose listings differ is reported symbol by symbol (identical / DIFFERENT, instruction counts of both builds), followed by
# the resource metadata of both code objects for every differing kernel (registers, spills, scratch and LDS bytes: what fixes the
# occupancy) and the first lines of the text difference.
set -u
A=$1; B=$2; shift 2
LLVM=${LLVM:-/opt/rocm/llvm/bin}
T=$(mktemp -d)
bad=0
# listing of one object into $2; returns 0 = device code listed, 2 = the object has no .hip_fatbin section, 1 = error
listing() {
  : > "$2"
  [ -f "$1" ] || { echo "missing object $1"; return 1; }
  "$LLVM/llvm-objdump" -h "$1" | grep -q "\.hip_fatbin" || return 2
  "$LLVM/llvm-objcopy" --dump-section .hip_fatbin="$2.fat" "$1" || return 1
  "$LLVM/clang-offload-bundler" --unbundle --type=o --targets=hipv4-amdgcn-amd-amdhsa--gfx950 --input="$2.fat" --output="$2.co" || return 1
  "$LLVM/llvm-objdump" -d "$2.co" | grep -v "file format" > "$2" || return 1
}
# splits a listing into one file per symbol under directory $2 and prints "symbol instruction-count" per symbol.  The symbol line
# and the instructions' addresses are left out, so a kernel that merely moved behind a changed one compares equal
per_symbol() {
  mkdir -p "$2"
  awk -v d="$2" '/^[0-9a-f]+ <.*>:$/ { if (name != "") print name, n; name = substr($2, 2, length($2) - 3); n = 0; next }
                 name != "" { if ($0 ~ /\/\/ [0-9A-F]+: /) ++n; sub(/\/\/ [0-9A-F]+: /, "// "); print > (d "/" name) }
                 END { if (name != "") print name, n }' "$1" | sort
}
# resource metadata of kernel $2 in code object $1, on one line
resources() {
  "$LLVM/llvm-readelf" --notes "$1" | awk -v k="$2" '
    function flush() { if (hit) print line; hit = 0; line = "" }
    /^ *- \.agpr_count:/ { flush(); line = " agpr_count:" $3; next }
    /^ *\.(vgpr_count|sgpr_count|vgpr_spill_count|sgpr_spill_count|private_segment_fixed_size|group_segment_fixed_size):/ { line = line " " substr($1, 2) $2 }
    /^ *\.name:/ && $2 == k { hit = 1 }
    END { flush() }'
}
units=("$@")
[ ${#units[@]} -gt 0 ] || for src in "$B"/*.hip; do units+=("$(basename "$src" .hip)"); done
for u in "${units[@]}"; do
  listing "$A/$u.o" "$T/$u.A.s"; ra=$?
  listing "$B/$u.o" "$T/$u.B.s"; rb=$?
  if [ $ra -eq 1 ] || [ $rb -eq 1 ]; then echo "$u.hip: ERROR (extraction failed)"; bad=1
  elif [ $ra -eq 2 ] && [ $rb -eq 2 ]; then echo "$u.hip: no device code in either object"
  elif [ $ra -ne $rb ]; then echo "$u.hip: DIFFERENT (device code in one object only)"; bad=1
  elif cmp -s "$T/$u.A.s" "$T/$u.B.s"; then
    echo "$u.hip: identical ($(grep -c "^[0-9a-f]* <.*>:$" "$T/$u.B.s") symbols, $(wc -l < "$T/$u.B.s") lines)"
  else
    echo "$u.hip: DIFFERENT ($(diff "$T/$u.A.s" "$T/$u.B.s" | grep -c '^[<>]') differing listing lines)"; bad=1
    per_symbol "$T/$u.A.s" "$T/$u.A.d" > "$T/$u.A.sym"
    per_symbol "$T/$u.B.s" "$T/$u.B.d" > "$T/$u.B.sym"
    join -a1 -a2 -e - -o 0,1.2,2.2 "$T/$u.A.sym" "$T/$u.B.sym" | while read -r sym na nb; do
      if cmp -s "$T/$u.A.d/$sym" "$T/$u.B.d/$sym"; then echo "  identical  $na instructions  $sym"
      else
        echo "  DIFFERENT  $na -> $nb instructions  $sym"
        echo "    parent:$(resources "$T/$u.A.s.co" "$sym")"
        echo "    new:   $(resources "$T/$u.B.s.co" "$sym")"
      fi
    done
    diff "$T/$u.A.s" "$T/$u.B.s" | head -20
  fi
done
rm -rf "$T"
exit $bad
