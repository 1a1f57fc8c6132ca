#!/bin/bash
# Device code of two builds, kernel by kernel: unbundles the gfx950 code object of every .hip unit's .o in two csrc directories,
# disassembles both and compares the text.  Needs no GPU.  A missing object or a failed extraction is an error, not "identical".
#   tools/device_code_ab.sh PARENT/pointreggpt_amd/csrc NEW/pointreggpt_amd/csrc [unit ...]      (units: names without .hip; default all)
# A unit whose listings differ is reported symbol by symbol (identical / DIFFERENT, instruction counts of both builds), followed by
# the resource metadata of both code objects for every differing kernel (registers, spills, scratch and LDS bytes: what fixes the
# occupancy) and the first lines of the text difference.
#   tools/device_code_ab.sh --by-symbol PARENT/pointreggpt_amd/csrc NEW/pointreggpt_amd/csrc
# For kernels that moved between units: the per-symbol listings of ALL units of each tree (each tree's own *.hip list) are pooled and
# compared symbol by symbol, whichever unit holds them.  Per symbol: identical, DIFFERENT (both instruction counts and the resource
# metadata) or present in one tree only (an error, like a difference); a symbol that two units of one tree both define is an error.
set -u
by_symbol=0
[ "${1:-}" = "--by-symbol" ] && { by_symbol=1; shift; }
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
# and the instructions' addresses are left out, so a kernel that merely moved behind a changed one compares equal.  With a prefix $3
# the files are named $3.1, $3.2, ... (mangled names can be longer than a file name) and the line ends with that name; the
# disassembler's padding behind the LAST symbol of a code object (a "..." line and a blank one) is then dropped: it follows
# whichever kernel comes last, not the kernel.
per_symbol() {
  mkdir -p "$2"
  awk -v d="$2" -v pre="${3:-}" '
    function done_sym() { if (name != "") print name, n, (pre != "" ? f : "") }
    /^[0-9a-f]+ <.*>:$/ { done_sym(); name = substr($2, 2, length($2) - 3); n = 0; held = ""; f = pre != "" ? pre "." ++k : name; next }
    name != "" && pre != "" && /^[ \t]*(\.\.\.)?[ \t]*$/ { held = held $0 "\n"; next }
    name != "" { if ($0 ~ /\/\/ [0-9A-F]+: /) ++n; sub(/\/\/ [0-9A-F]+: /, "// "); printf "%s", held > (d "/" f); held = ""; print > (d "/" f) }
    END { done_sym() }' "$1" | sort
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
# every unit of tree $1 (letter $2) into the pool $T/$2.d; $T/$2.sym: "symbol instruction-count file unit", sorted by symbol
pool() {
  : > "$T/$2.sym"
  for src in "$1"/*.hip; do
    local u; u=$(basename "$src" .hip)
    listing "$1/$u.o" "$T/$u.$2.s"; local r=$?
    [ $r -eq 2 ] && continue
    [ $r -eq 0 ] || { echo "$u.hip: ERROR (extraction failed)"; bad=1; continue; }
    per_symbol "$T/$u.$2.s" "$T/$2.d" "$u" | sed "s/\$/ $u/" >> "$T/$2.sym"
  done
  sort -o "$T/$2.sym" "$T/$2.sym"
  local dup; dup=$(cut -d' ' -f1 "$T/$2.sym" | uniq -d)
  [ -z "$dup" ] || { echo "ERROR: defined by two units of $1:"; echo "$dup"; bad=1; }
}
if [ $by_symbol -eq 1 ]; then
  pool "$A" A; pool "$B" B
  while read -r sym na fa ua nb fb ub; do
    if [ "$na" = - ]; then echo "only in new     $nb instructions  $ub.hip  $sym"
    elif [ "$nb" = - ]; then echo "only in parent  $na instructions  $ua.hip  $sym"
    else
      where=$ub.hip; [ "$ua" = "$ub" ] || where="$ua.hip -> $ub.hip"
      if cmp -s "$T/A.d/$fa" "$T/B.d/$fb"; then echo "identical  $na instructions  $where  $sym"
      else
        echo "DIFFERENT  $na -> $nb instructions  $where  $sym"
        echo "    parent:$(resources "$T/$ua.A.s.co" "$sym")"
        echo "    new:   $(resources "$T/$ub.B.s.co" "$sym")"
      fi
    fi
  done < <(join -a1 -a2 -e - -o 0,1.2,1.3,1.4,2.2,2.3,2.4 "$T/A.sym" "$T/B.sym") > "$T/report"
  cat "$T/report"
  same=$(grep -c '^identical' "$T/report"); diff=$(grep -c '^DIFFERENT' "$T/report"); lone=$(grep -c '^only in' "$T/report")
  echo "$same symbols identical, $diff different, $lone in one tree only"
  [ "$diff" -eq 0 ] && [ "$lone" -eq 0 ] || bad=1
  rm -rf "$T"
  exit $bad
fi
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
