#!/bin/bash
# one md5 per kernel of the gfx950 device code of every .hip source in a directory (device-only compile, disassembly without
# addresses and encodings): diff two trees' lists to show which kernels' ISA changed.
# usage: tools/isa_hash.sh ssd_tensorflow_amd/csrc > new.txt ; (same on the parent's tree) > old.txt ; diff old.txt new.txt
src=${1:-ssd_tensorflow_amd/csrc}; tmp=$(mktemp -d)
for f in "$src"/*.hip; do
  b=$(basename "$f" .hip); extra=""; case $b in boxes|metrics|augment|annotate|planner) extra=-ffp-contract=off;; esac
  hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC $extra --cuda-device-only --no-gpu-bundle-output -c "$f" -o "$tmp/$b.co" &
done
wait
for c in "$tmp"/*.co; do
  /opt/rocm/llvm/bin/llvm-objdump -d --no-show-raw-insn "$c" | awk -v f="$(basename "$c" .co)" '
    /^[0-9a-f]+ <.*>:$/ {if (name != "") print f, name, body; name = $2; body = ""; next}
    name != "" && NF {sub(/^[ \t]*/, ""); sub(/\/\/.*$/, ""); body = body "|" $0}
    END {if (name != "") print f, name, body}' |
  while read -r f n b; do echo "$f $n $(echo "$b" | md5sum | cut -c1-12)"; done
done | sort
rm -rf "$tmp"
