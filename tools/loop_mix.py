#!/usr/bin/env python3
"""Instruction histogram of a kernel's K loop(s), from the compiler's assembly — no GPU needed.

    python tools/loop_mix.py e4s2024_amd/csrc/modconv_mx.hip 'region_modconv_mx_kernel<1, false, false, false>'
    python tools/loop_mix.py e4s2024_amd/csrc/modconv_mx4.hip region_upconv_mx4_kernel [-D...]

Compiles the file with the library's flags (e4s2024_amd/build.py) to device assembly, finds the kernel whose demangled name contains the given text, and for
every natural loop of it that holds matrix instructions prints the mnemonic counts of one trip, grouped: matrix,
vector ALU, LDS, vector memory, scalar, waits.  Also the kernel's register and spill counts.  A plain count of what one trip issues, nothing more."""
import collections
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from e4s2024_amd import build as B  # noqa: E402

CXXFILT = "c++filt"


def assembly(src, extra):
    cmd = [B.HIPCC] + [f for f in B.FLAGS if f != "-fPIC"] + list(extra) + ["-S", "--cuda-device-only", src, "-o", "-"]
    res = subprocess.run(cmd, capture_output=True, text=True)
    if res.returncode != 0:
        sys.exit(res.stderr)
    return res.stdout


def kernels(asm):
    """mangled name -> its lines (from the label to .Lfunc_end)."""
    out, name, cur = {}, None, None
    for line in asm.splitlines():
        m = re.match(r"^(_Z\w+|[A-Za-z_]\w*):\s*(;.*)?$", line)
        if m and name is None and not line.startswith(".L"):
            name, cur = m.group(1), []
            continue
        if name is not None:
            if line.startswith(".Lfunc_end"):
                out[name] = cur
                name = None
            else:
                cur.append(line)
    return out


def demangle(names):
    try:
        res = subprocess.run([CXXFILT], input="\n".join(names), check=True, capture_output=True, text=True).stdout.splitlines()
        return dict(zip(names, res))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def group(mn):
    if mn.startswith("v_mfma") or mn.startswith("v_smfma"):
        return "matrix"
    if mn.startswith("ds_"):
        return "lds"
    if mn.startswith(("global_", "buffer_", "flat_", "scratch_")):
        return "vmem"
    if mn.startswith("s_waitcnt") or mn == "s_barrier" or mn == "s_nop":
        return "wait"
    if mn.startswith("v_"):
        return "valu"
    return "scalar"


def loops(lines):
    """Natural loops of the kernel's control-flow graph: [(header label, body lines in program order)], loops that share a header merged.  Blocks are cut at labels and
    behind branches; a back edge is an edge to a block that dominates its source (block layout interleaves the bodies of different loops and does not put a header
    first, so a label-to-branch line range is not a loop)."""
    starts, label_at = [0], {}
    for i, line in enumerate(lines):
        m = re.match(r"^(\.LBB\w+):", line)
        if m:
            label_at[m.group(1)] = i
            starts.append(i)
        elif re.match(r"^\s+(s_c?branch\w*|s_endpgm|s_setpc\w*)\b", line):
            starts.append(i + 1)
    starts = sorted(set(s for s in starts if s < len(lines)))
    block_of = {s: k for k, s in enumerate(starts)}
    ends = starts[1:] + [len(lines)]
    succ = [[] for _ in starts]
    for k, (s, e) in enumerate(zip(starts, ends)):
        last = next((ln for ln in reversed(lines[s:e]) if re.match(r"^\s+[a-z]", ln)), "")
        m = re.match(r"^\s+(s_c?branch\w*)\s+(\.LBB\w+)", last)
        if m and m.group(2) in label_at:
            succ[k].append(block_of[label_at[m.group(2)]])
        if not re.match(r"^\s+(s_branch|s_endpgm|s_setpc\w*)\b", last) and k + 1 < len(starts):
            succ[k].append(k + 1)
    pred = [[] for _ in starts]
    for k, ss in enumerate(succ):
        for j in ss:
            pred[j].append(k)
    n = len(starts)
    dom = [set(range(n)) for _ in range(n)]        # iterative dominator sets (a few hundred blocks)
    dom[0] = {0}
    changed = True
    while changed:
        changed = False
        for k in range(1, n):
            ps = [dom[q] for q in pred[k]]
            d = (set.intersection(*ps) if ps else set()) | {k}
            if d != dom[k]:
                dom[k], changed = d, True
    bodies = {}
    for k, ss in enumerate(succ):
        for h in ss:
            if h not in dom[k]:           # a back edge goes to a block that dominates its source
                continue
            body, todo = {h}, [k]
            while todo:
                q = todo.pop()
                if q not in body:
                    body.add(q)
                    todo.extend(pred[q])
            bodies.setdefault(h, set()).update(body)
    out = []
    for h, body in sorted(bodies.items()):
        text = [ln for k in sorted(body) for ln in lines[starts[k]:ends[k]]]
        out.append((lines[starts[h]].split(":")[0], body, text))
    return out


def histogram(lines):
    h = collections.Counter()
    for line in lines:
        m = re.match(r"^\s+([a-z]\w+)", line)
        if m and not line.lstrip().startswith((".", ";")):
            h[m.group(1)] += 1
    return h


def mov_feeds_mfma(lines):
    """v_mov_b32 whose destination register lies in the A / B operand range of a LATER matrix instruction of the trip, not rewritten in between (a count of operand
    marshaling moves; accumulator initialisation does not count: operand 3 is not looked at)."""
    n = 0
    for i, line in enumerate(lines):
        m = re.match(r"^\s+v_mov_b32(?:_e32)?\s+v(\d+),", line)
        if not m:
            continue
        r = int(m.group(1))
        for later in lines[i + 1:]:
            mm = re.match(r"^\s+(\w+)\s+(.*)$", later)
            if not mm:
                continue
            ops_ = mm.group(2).split(";")[0]
            if mm.group(1).startswith("v_mfma"):
                rng = re.findall(r"v\[(\d+):(\d+)\]", ops_)
                if any(int(a) <= r <= int(b) for a, b in rng[1:3]):
                    n += 1
                    break
            dst = re.match(r"\s*v(\d+)\b|\s*v\[(\d+):(\d+)\]", ops_)
            if dst and ((dst.group(1) and int(dst.group(1)) == r) or (dst.group(2) and int(dst.group(2)) <= r <= int(dst.group(3)))):
                break
    return n


def main():
    if len(sys.argv) < 3:
        sys.exit(__doc__)
    src, want, extra = sys.argv[1], sys.argv[2], sys.argv[3:]
    asm = assembly(src, extra)
    ks = kernels(asm)
    names = demangle(list(ks))
    hits = [n for n in ks if want in names[n] or want in n]
    if not hits:
        sys.exit(f"no kernel matches {want!r}; kernels: " + "; ".join(sorted(set(names.values()))))
    for n in hits:
        lines = ks[n]
        print(f"== {names[n]}  ({os.path.basename(src)})")
        for key in (".vgpr_count", ".agpr_count", ".vgpr_spill_count", ".sgpr_spill_count", ".private_segment_fixed_size"):
            m = re.search(r"\.name:\s+" + re.escape(n) + r"\b.*?" + re.escape(key) + r":\s+(\d+)", asm, re.S) or \
                re.search(re.escape(key) + r":\s+(\d+)(?=(?:(?!\.name:).)*\.name:\s+" + re.escape(n) + r"\b)", asm, re.S)
            print(f"   {key[1:]:28s} {m.group(1) if m else '?'}")
        found = loops(lines)
        for lab, blocks, body in found:
            h = histogram(body)
            nm = sum(c for mn, c in h.items() if group(mn) == "matrix")
            if nm == 0:
                continue
            inner = [x for x in found if x[1] < blocks]
            by = collections.defaultdict(int)
            for mn, c in h.items():
                by[group(mn)] += c
            print(f"-- loop {lab}: {len(blocks)} blocks, {sum(h.values())} instructions per trip" + (f"  (contains {len(inner)} inner loop(s))" if inner else ""))
            print("   " + "  ".join(f"{g} {by[g]}" for g in ("matrix", "valu", "lds", "vmem", "scalar", "wait")))
            print(f"   v_mov_b32 feeding a matrix operand: {mov_feeds_mfma(body)}")
            for g in ("matrix", "valu", "lds", "vmem", "wait", "scalar"):
                items = sorted(((c, mn) for mn, c in h.items() if group(mn) == g), reverse=True)
                if items:
                    print(f"   [{g}] " + ", ".join(f"{mn} {c}" for c, mn in items))


if __name__ == "__main__":
    main()
