"""Run the C2 forward with the stamp build and print per-section wave cycles (mean per launch).
Usage (GPU box): NONODE_LIB=no-node-comparison_amd/libnonode_stamp.so python3 tools/stamp_run.py"""
import ctypes
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import bench  # noqa: E402
import no_node_comparison_amd as pkg  # noqa: E402
from no_node_comparison_amd import _lib  # noqa: E402

NAMES = {0: "B pair head", 1: "B pair silu/split/mfma W2", 2: "B pair silu/split/mfma Wc1", 3: "B pair tail",
         4: "B triple iteration", 5: "B segment prologue", 14: "B single unit", 6: "A work",
         7: "A barrier", 8: "B singles prologue", 9: "B flush", 10: "B end (last seg)", 11: "B barrier",
         12: "C work", 13: "C barrier",
         # the tile-segment boundary taken apart (round 8): 16 + 17 + 18 + 5 were bucket 5, 19 + 4 bucket 4
         16: "B chunk preamble", 17: "B segment state", 18: "B fragment reads landed", 19: "B first triple of a segment"}
NAMES[5] = "B segment prologue (rest)"
dev = torch.device("cuda:0")
torch.manual_seed(0)
model = pkg.EGNO(n_layers=4, in_node_nf=2, in_edge_nf=2, hidden_nf=64, with_v=True, num_modes=2,
                 num_timesteps=10, time_emb_dim=32, device=dev).eval()
case = bench.build_egno_case(512, 20, 10, seed=1234, dev=dev)
L = _lib.lib()
buf = (ctypes.c_ulonglong * 24)()
with torch.no_grad():
    for it in range(3):
        model(case["x"], case["h"], case["edges"], case["edge_fea"], v=case["v"], loc_mean=case["loc_mean"],
              timesteps_out=case["t_out"])
        torch.cuda.synchronize()
        assert L.nonode_debug_stamps(buf) == 0
launches = 4
waves = 256 * int(os.environ.get("NONODE_WAVES", "8"))
tot = sum(buf)
for i in range(24):
    if buf[i]:
        print(f"{i:2d} {NAMES.get(i, '?'):28s} {buf[i] / launches / waves:10.0f} cyc/wave/launch  {buf[i] / tot:6.1%}")
print(f"   total {tot / launches / waves:.0f} cyc/wave/launch")
# cycles per iteration of the edge walk (the constants of the split's cost model, nonode_common.h):
# the walk of this build's C2 chunk (4 graphs, 5 full tiles of 19 units) from the library itself
cut = (ctypes.c_int * 5)()
rows = (ctypes.c_int * (8 * 64))()
nseg = L.nonode_debug_edge_walk(0, 5, 19, 19, 19, cut, rows, 64)
tri, pair, one = (sum(rows[8 * i + j] for i in range(nseg)) for j in (4, 5, 6))
chunks = launches * (512 * 10 // 4)
print(f"   C2 chunk: cuts {list(cut)}, {nseg} segments, {tri} triples, {pair} pairs, {one} singles")
for name, cyc, n in (("segment (prologue + flush)", buf[16] + buf[17] + buf[18] + buf[5] + buf[8] + buf[9], nseg),
                     ("first triple of a segment", buf[19], sum(1 for i in range(nseg) if rows[8 * i + 4])),
                     ("later triple", buf[4], tri - sum(1 for i in range(nseg) if rows[8 * i + 4])),
                     ("pair", buf[0] + buf[1] + buf[2] + buf[3], pair), ("single", buf[14], one)):
    if n:
        print(f"   {name:28s} {cyc / chunks / n:8.0f} cycles each")
