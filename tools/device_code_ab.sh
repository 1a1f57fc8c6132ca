#!/bin/bash
# Device code of two builds, kernel by kernel: unbundles the gfx950 code object of every .hip unit's .o in two csrc directories,
# disassembles both and compares the text.  Needs no GPU.  A missing object or a failed extraction is an error, not "identical".
#   tools/device_code_ab.sh PARENT/pointreggpt_amd/csrc NEW/pointreggpt_amd/csrc
set -u
A=$1; B=$2
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
for src in "$B"/*.hip; do
  u=$(basename "$src" .hip)
  listing "$A/$u.o" "$T/$u.A.s"; ra=$?
  listing "$B/$u.o" "$T/$u.B.s"; rb=$?
  if [ $ra -eq 1 ] || [ $rb -eq 1 ]; then echo "$u.hip: ERROR (extraction failed)"; bad=1
  elif [ $ra -eq 2 ] && [ $rb -eq 2 ]; then echo "$u.hip: no device code in either object"
  elif [ $ra -ne $rb ]; then echo "$u.hip: DIFFERENT (device code in one object only)"; bad=1
  elif cmp -s "$T/$u.A.s" "$T/$u.B.s"; then
    echo "$u.hip: identical ($(grep -c "^[0-9a-f]* <.*>:$" "$T/$u.B.s") symbols, $(wc -l < "$T/$u.B.s") lines)"
  else echo "$u.hip: DIFFERENT"; diff "$T/$u.A.s" "$T/$u.B.s" | head -20; bad=1; fi
done
rm -rf "$T"
exit $bad
