#!/bin/bash
# device assembly of one translation unit, with the command build() compiles it with
# (__graft_entry__.compile_cmd): bash tools/isa.sh <out.s> [-DFLAG=VAL ...]
# UNIT=nonode_node.hip for another unit; NONODE_SCHED=... overrides nonode.hip's machine scheduler
cd "$(dirname "$0")/.."
out=$1; shift
exec $(python3 -c "import sys; import __graft_entry__ as g; print(' '.join(g.compile_cmd(sys.argv[1], sys.argv[2], sys.argv[3:], asm=True)))" "${UNIT:-nonode.hip}" "$out" "$@")
