"""Instruction budget of the EGNO four-wave layer kernel's hot edge blocks, per edge unit and by
category, from a device assembly file (tools/isa.sh output), plus the kernel's registers and scratch.

python tools/isa_budget.py a.s [--kernel substr]

The triple block is the basic block of egnn_layer_kernel<EGNO, KF=1, 4 waves> with three units'
transcendentals (3 SiLUs of 16 values each: 144 v_exp_f32) and 156 MFMAs, the pair block the one with
two units' (96, 104); the first of each (the default-option copy of the body) is printed."""
import collections
import re
import sys

sys.path.insert(0, __import__("os").path.dirname(__import__("os").path.abspath(__file__)))
import isa_stats  # noqa: E402

KERNEL = "egnn_layer_kernelILi0ELi1ELi4E"
CATEGORIES = ("transcendental", "SiLU arithmetic", "split", "MFMA f16", "MFMA f32", "in-place adds", "dot",
              "moves + accvgpr", "integer/address/compare", "LDS", "global", "waits/nops", "other")


def category(op, args):
    if op in ("v_exp_f32_e32", "v_rcp_f32_e32", "v_exp_f32", "v_rcp_f32"):
        return "transcendental"
    if op.startswith("v_mfma"):
        return "MFMA f16" if op.endswith("_f16") else "MFMA f32"
    if op.startswith(("v_cvt_pk_f16_f32", "v_fma_mix", "v_pk_mul_f16")):
        return "split"
    if op.startswith("v_add_f32"):
        # SiLU's 1 + 2^z carries the inline constant; every other f32 add is a P + Q, pair or message sum
        return "SiLU arithmetic" if re.search(r"(^|,\s*)1\.0(,|$)", args) else "in-place adds"
    if op.startswith("v_mul_f32"):
        return "SiLU arithmetic"     # z * r (and the few |r|^2 / r * c products of the head and tail)
    if op.startswith(("v_fmac_f32", "v_fma_f32", "v_pk_fma_f32")):
        return "dot"
    if op.startswith(("v_mov", "v_accvgpr", "v_permlane", "v_swap")):
        return "moves + accvgpr"
    if op.startswith("ds_"):
        return "LDS"
    if op.startswith(("global_", "buffer_", "scratch_", "flat_")):
        return "global"
    if op.startswith(("s_waitcnt", "s_nop", "s_barrier", "s_sleep")):
        return "waits/nops"
    if op.startswith(("s_", "v_cmp", "v_cndmask", "v_add_u32", "v_sub_u32", "v_add_co", "v_addc", "v_lshl", "v_lshr",
                      "v_ashr", "v_and", "v_or", "v_xor", "v_mad_u", "v_mad_i", "v_mul_lo", "v_mul_hi", "v_min_", "v_max_",
                      "v_add3", "v_add_lshl", "v_lshl_add", "v_lshl_or", "v_and_or", "v_bfe", "v_readfirstlane",
                      "v_sub_co", "v_subrev", "v_sub_nc", "v_add_nc", "v_med3", "v_mbcnt", "v_bfi", "v_not")):
        return "integer/address/compare"
    return "other"


def basic_blocks(body):
    """[(label, [(opcode, operands)])] of a kernel body, split at labels and after branches."""
    out, cur, name = [], [], "entry"
    for ln in body:
        m = re.match(r"^(\.LBB\S+):", ln)
        if m:
            if cur:
                out.append((name, cur))
            name, cur = m.group(1), []
            continue
        if not ln.startswith("\t") or ln.startswith(("\t.", "\t;")):
            continue
        parts = ln.split(";")[0].split(None, 1)
        if not parts:
            continue
        cur.append((parts[0], parts[1].strip() if len(parts) > 1 else ""))
        if parts[0].startswith(("s_cbranch", "s_branch", "s_endpgm")):
            out.append((name, cur))
            name, cur = name + "+", []
    if cur:
        out.append((name, cur))
    return out


def hot_blocks(body):
    """{'triple': block, 'pair': block}: the first basic blocks with 144 / 96 v_exp_f32 and 156 / 104 MFMAs."""
    found = {}
    for name, ins in basic_blocks(body):
        nexp = sum(op.startswith("v_exp_f32") for op, _ in ins)
        nmf = sum(op.startswith("v_mfma") for op, _ in ins)
        for key, units in (("triple", 3), ("pair", 2)):
            if nexp == 48 * units and nmf == 52 * units and key not in found:
                found[key] = (name, ins)
    return found


def budget(path, kernel=KERNEL):
    ks = isa_stats.kernels(path)
    names = [k for k in ks if kernel in k]
    if len(names) != 1:
        raise SystemExit(f"{path}: {len(names)} kernels match {kernel!r}")
    k = ks[names[0]]
    res = {"kernel": names[0], "vgpr": k["num_vgpr"], "agpr": k["num_agpr"], "scratch": k["private_seg_size"],
           "instructions": k["n"], "blocks": {}}
    for key, (name, ins) in hot_blocks(k["body"]).items():
        units = 3 if key == "triple" else 2
        cnt = collections.Counter(category(op, args) for op, args in ins)
        other = collections.Counter(op for op, args in ins if category(op, args) == "other")
        res["blocks"][key] = {"label": name, "units": units, "n": len(ins), "by_category": cnt, "other_ops": other}
    return res


def main():
    files = [a for a in sys.argv[1:] if not a.startswith("--")]
    kernel = sys.argv[sys.argv.index("--kernel") + 1] if "--kernel" in sys.argv else KERNEL
    files = [f for f in files if f != kernel]
    for f in files:
        r = budget(f, kernel)
        print(f"{r['kernel']}: {r['instructions']} instructions, vgpr {r['vgpr']} agpr {r['agpr']} scratch {r['scratch']} bytes")
        for key in ("triple", "pair"):
            b = r["blocks"].get(key)
            if b is None:
                print(f"  {key} block: not found")
                continue
            print(f"  {key} block {b['label']}: {b['n']} instructions, {b['n'] / b['units']:.1f} per unit")
            for c in CATEGORIES:
                if b["by_category"].get(c):
                    print(f"    {c:26s} {b['by_category'][c]:5d}  {b['by_category'][c] / b['units']:7.1f} per unit")
            if b["other_ops"]:
                print("    (other: " + ", ".join(f"{o} {n}" for o, n in sorted(b["other_ops"].items())) + ")")


if __name__ == "__main__":
    main()
