"""Static instruction mix of the factorisation's node loop (no GPU needed).

Compiles solve.hip with build.py's flags to gfx950 assembly, finds the depth-1 loop of the one-wave riccati_factor
(the blocks the compiler marks `in Loop: Header=...`; the loop with the most instructions if there are several) and
prints its instruction count by kind, then solve_kernel's VGPR / spill / scratch / LDS figures from the code object
metadata.

    python profiles/tools/isa_loop_mix.py [--src mpconstellation_amd/csrc/solve.hip] [--asm FILE] [--keep FILE.s]

With --func NAME / --kernel NAME (both repeatable, any translation unit of the solver) it prints instead one line per function
-- instructions of the whole body: total, fp64, LDS, scratch, s_waitcnt -- and one per kernel -- VGPRs, AGPRs, VGPR and SGPR
spills, scratch bytes, static LDS from the code object metadata:

    python profiles/tools/isa_loop_mix.py --src mpconstellation_amd/csrc/solve2w.hip --func riccati_factor2 --kernel solve_kernel2w
"""
import argparse
import collections
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

FUNC = "_ZN4mpcx14riccati_factor"
KERNEL = "_ZN4mpcx12solve_kernelENS_9SolveArgsE"

# first matching rule wins
KINDS = [
    ("scratch", r"^scratch_"),
    ("wait/nop", r"^s_(waitcnt|nop|sleep|barrier)|^s_wait_"),
    ("branch", r"^s_(cbranch|branch|setpc|swappc|getpc)"),
    ("exec-mask", r"^s_\w+_saveexec_b64|^s_\w+_b64 exec,"),
    ("lane read/write", r"^v_(readlane|readfirstlane|writelane)"),
    ("fp64", r"^v_\w*_f64|^v_(fma|fmac|mul|add|min|max|rcp|rsq|sqrt|div_\w+|ldexp|frexp\w*|cmp\w*|trig_preop)_f64"),
    ("LDS", r"^ds_"),
    ("vector memory", r"^(global|buffer|flat)_"),
    ("scalar memory", r"^s_(load|buffer_load)"),
    ("move", r"^v_(mov|accvgpr)"),
    ("cndmask", r"^v_cndmask"),
    ("integer/address", r"^v_(add|sub|lshl|lshr|ashr|mad|mul|and|or|xor|bfe|bfi|alignbit|perm|cmp|min|max|not|lshl_add|add3|or3)"),
    ("scalar", r"^s_"),
    ("other vector", r"^v_"),
]
KINDS = [(n, re.compile(p)) for n, p in KINDS]


def compile_asm(src, out):
    from mpconstellation_amd import build as b
    flags = [f for f in b.FLAGS if f not in ("-shared", "-fPIC", "-pthread")]
    cmd = [b.HIPCC] + flags + ["--cuda-device-only", "-S", "-o", out, src]
    subprocess.check_call(cmd, stderr=subprocess.DEVNULL)


def function_lines(lines, name_prefix):
    start = end = None
    for i, ln in enumerate(lines):
        if start is None and re.match(r"^" + re.escape(name_prefix) + r"\S*:", ln):
            start = i
        elif start is not None and ln.lstrip().startswith(".Lfunc_end"):
            end = i
            break
    if start is None:
        sys.exit(f"function {name_prefix}* not found")
    return lines[start:end]


def loops(body):
    """{header: [instruction, ...]} of the depth-1 loops (nested loops' blocks are counted with the outer loop they sit in)."""
    out = collections.OrderedDict()
    cur = None          # header of the depth-1 loop the current block belongs to
    for ln in body:
        m = re.match(r"^(\.LBB\w+|; %bb\.\d+):\s*(;.*)?$", ln)
        if m:
            com = m.group(2) or ""
            h = re.search(r"=>This (Inner )?Loop Header: Depth=(\d+)", com)
            il = re.search(r"in Loop: Header=(\w+) Depth=(\d+)", com)
            if h and h.group(2) == "1":
                cur = m.group(1).lstrip(".")
            elif il and il.group(2) == "1":
                cur = il.group(1)
            elif h or il:
                pass        # a nested block: stays with the enclosing depth-1 loop
            else:
                cur = None
            if cur is not None:
                out.setdefault(cur, [])
            continue
        s = ln.strip()
        if cur is None or not s or s.startswith((";", ".")) or s.endswith(":"):
            continue
        out[cur].append(s.split(";")[0].strip())
    return out


def classify(ins):
    op = ins.split()[0]
    for name, rx in KINDS:
        if rx.search(op if name != "exec-mask" else ins):
            return name
    return "other"


def function_figures(lines, name):
    """(mangled name, counts) of the function `name` of the solver's namespace (mpcx, mpcx2w, mpcxl, mpcxtp), lambdas apart"""
    rx = re.compile(r"^(_ZN\d+mpcx\w*?%d%sE\S*):" % (len(name), re.escape(name)))
    for ln in lines:
        m = rx.match(ln)
        if m:
            break
    else:
        sys.exit(f"function {name} not found")
    ins = [l.strip().split(";")[0].strip() for l in function_lines(lines, m.group(1))[1:]]
    ins = [i for i in ins if i and not i.startswith(".") and not i.endswith(":")]
    mix = collections.Counter(classify(i) for i in ins)
    return {"total": len(ins), "fp64": mix["fp64"], "LDS": mix["LDS"], "scratch": mix["scratch"],
            "s_waitcnt": sum(1 for i in ins if i.startswith("s_waitcnt"))}


def kernel_meta(text, kernel=KERNEL):
    """code object metadata of a kernel, by its mangled name or by its plain name in the solver's namespace"""
    m = re.search(r"\.name:\s+(" + re.escape(kernel) + r"|_ZN\d+mpcx\w*?%d%sE\S*)\s*$" % (len(kernel), re.escape(kernel)), text, re.M)
    if not m:
        return {}
    # the metadata map of one kernel: from its "  - ." line to the next kernel's
    a = text.rfind("\n  - .", 0, m.start())
    b = text.find("\n  - .", m.end())
    blk = text[a:b if b > 0 else len(text)]
    meta = {}
    for key in ("vgpr_count", "vgpr_spill_count", "sgpr_count", "sgpr_spill_count", "private_segment_fixed_size",
                "group_segment_fixed_size", "agpr_count"):
        mm = re.search(r"\." + key + r":\s+(\d+)", blk)
        if mm:
            meta[key] = int(mm.group(1))
    return meta


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--src", default=os.path.join(ROOT, "mpconstellation_amd", "csrc", "solve.hip"))
    ap.add_argument("--asm", help="read this assembly file instead of compiling")
    ap.add_argument("--keep", help="keep the compiled assembly here")
    ap.add_argument("--func", action="append", default=[], help="whole-function instruction counts of this function")
    ap.add_argument("--kernel", action="append", default=[], help="register / spill / scratch / LDS figures of this kernel")
    args = ap.parse_args()
    if args.asm:
        path = args.asm
    else:
        path = args.keep or os.path.join(tempfile.mkdtemp(), "solve.s")
        compile_asm(args.src, path)
    text = open(path).read()
    lines = text.splitlines()
    if args.func or args.kernel:
        for name in args.func:
            f = function_figures(lines, name)
            print(f"{name}: " + ", ".join(f"{k} {v}" for k, v in f.items()))
        for name in args.kernel:
            meta = kernel_meta(text, name)
            if not meta:
                sys.exit(f"kernel {name} not found")
            print(f"{name}: VGPRs {meta.get('vgpr_count')}, AGPRs {meta.get('agpr_count', 0)}, VGPR spills {meta.get('vgpr_spill_count')}, "
                  f"SGPR spills {meta.get('sgpr_spill_count')}, scratch {meta.get('private_segment_fixed_size')} B, "
                  f"LDS {meta.get('group_segment_fixed_size')} B")
        return
    body = function_lines(lines, FUNC)
    lp = loops(body)
    if not lp:
        sys.exit("no depth-1 loop in riccati_factor")
    header, ins = max(lp.items(), key=lambda kv: len(kv[1]))
    mix = collections.Counter(classify(i) for i in ins)
    print(f"riccati_factor node loop (header {header}): {len(ins)} instructions")
    for name, _ in KINDS + [("other", None)]:
        if mix.get(name):
            print(f"  {name:18s} {mix[name]:5d}")
    dpp = sum(1 for i in ins if i.startswith("v_mov_b64_dpp"))
    sx = sum(1 for i in ins if re.match(r"s_(and|or|xor|andn2)_saveexec", i))
    print(f"  (v_mov_b64_dpp {dpp}, saveexec regions {sx}, "
          f"ds_read_b128/read2 {sum(1 for i in ins if re.match(r'ds_read(_b128|2)', i))})")
    scr = [i for i in ins if i.startswith("scratch_")]
    print(f"  scratch instructions in the loop: {len(scr)}")
    meta = kernel_meta(text)
    print(f"solve_kernel: VGPRs {meta.get('vgpr_count')}, VGPR spills {meta.get('vgpr_spill_count')}, "
          f"SGPR spills {meta.get('sgpr_spill_count')}, scratch {meta.get('private_segment_fixed_size')} B, "
          f"LDS {meta.get('group_segment_fixed_size')} B")
    for name, lo in (("VGPRs", meta.get("vgpr_count", 0) <= 256), ("LDS", meta.get("group_segment_fixed_size", 0) <= 20480),
                     ("loop scratch", not scr)):
        if not lo:
            print(f"  WARNING: {name} outside the limits (256 VGPRs, 20480 B LDS, no scratch in the loop)")


if __name__ == "__main__":
    main()
