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

With --driver FUNCTION (a kernel or a device function; every instantiation of a template) it prints the spill traffic of the
function's own body: per loop depth the instructions, the scratch loads and stores by stack offset, the full vmcnt(0) waits, the
lane moves of the SGPR spills and the calls; then the whole-body spill figures of every function of the translation unit that has
any (scratch instructions, lane moves, spilled VGPR dwords, SGPR spill lanes).  The code object metadata that --kernel prints
counts a kernel's own body only, not the functions it calls (profiles/solve_spill_traffic.txt):

    python profiles/tools/isa_loop_mix.py --driver solve_kernel --driver ipm_iterate --kernel solve_kernel
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


def blocks_by_depth(body):
    """[(loop depth, [instruction, ...]), ...] of a function's basic blocks, from the compiler's block annotations
    (`=>This Loop Header: Depth=n`, which may stand on a comment line of its own behind the label, and `in Loop: Header=... Depth=n`)"""
    out = []
    fresh = False       # the last line was a block label or one of its comment lines
    for ln in body:
        m = re.match(r"^(\.LBB\w+|; %bb\.\d+):\s*(;.*)?$", ln)
        if m:
            out.append([0, []])
            fresh = True
        elif not (fresh and re.match(r"^\s+;", ln)):
            fresh = False
        if fresh and out:
            d = re.search(r"Loop Header: Depth=(\d+)|in Loop: Header=\w+ Depth=(\d+)", ln)
            if d:
                out[-1][0] = int(d.group(1) or d.group(2))
            continue
        s = ln.strip()
        if not out or not s or s.startswith((";", ".")) or s.endswith(":"):
            continue
        out[-1][1].append(s.split(";")[0].strip())
    return out


def scratch_offset(ins):
    m = re.search(r"offset:(\d+)", ins)
    return int(m.group(1)) if m else 0


def short_name(mangled):
    ns = re.match(r"^_ZN(\d+)", mangled)                    # _ZN <length> namespace <length> name ...
    dm = re.compile(r"(\d+)").match(mangled, ns.end() + int(ns.group(1)))
    n = int(dm.group(1))
    return mangled[dm.end():dm.end() + n] + ("<1>" if "ILb1E" in mangled else "<0>" if "ILb0E" in mangled else "")


def spill_figures(raw):
    """whole body of one function from its assembly lines: scratch instructions, lane moves, and the spill slots they serve --
    dwords of the distinct stack offsets the compiler marks `Folded Spill`, distinct (register, lane) targets of v_writelane"""
    ins = [l.strip() for l in raw]
    slots, lanes = {}, set()
    for i in ins:
        m = re.match(r"scratch_store_dword(x(\d))?\b.*Folded Spill", i)
        if m:
            slots[scratch_offset(i)] = int(m.group(2) or 1)
        m = re.match(r"v_writelane_b32 (v\d+), \S+ (\d+)", i)
        if m:
            lanes.add(m.groups())
    return {"scratch": sum(1 for i in ins if i.startswith("scratch_")),
            "lane moves": sum(1 for i in ins if re.match(r"v_(readlane|writelane)", i)),
            "VGPR spill dwords": sum(slots.values()), "SGPR spill lanes": len(lanes)}


def driver_census(lines, func):
    """Spill traffic of a function's own body per loop depth -- a kernel (its driver, inlined) or a device function, every
    instantiation if it is a template -- then its whole-body spill figures and those of every out-of-line function of the
    translation unit.  A kernel's code object metadata (--kernel) counts the spills of the kernel's own body only: the functions
    it calls are in this table."""
    rx = re.compile(r"^(_ZN\d+mpcx\w*?%d%s[EI]\S*):" % (len(func), re.escape(func)))
    names = [rx.match(l).group(1) for l in lines if rx.match(l)]
    if not names:
        sys.exit(f"function {func} not found")
    for name in names:
        raw = function_lines(lines, name)[1:]
        blocks = blocks_by_depth(raw)
        print(f"{short_name(name)}: the function's own body by loop depth")
        loops_ld = loops_wait = 0
        for depth in sorted({d for d, _ in blocks}):
            ins = [i for d, b in blocks if d == depth for i in b]
            ld = collections.Counter(scratch_offset(i) for i in ins if i.startswith("scratch_load"))
            st = collections.Counter(scratch_offset(i) for i in ins if i.startswith("scratch_store"))
            waits = sum(1 for i in ins if re.match(r"s_waitcnt .*vmcnt[(]0[)]", i))
            print(f"  depth {depth}: {len(ins)} instructions, scratch loads {sum(ld.values())}, scratch stores {sum(st.values())}, "
                  f"vmcnt(0) waits {waits}, "
                  f"v_readlane {sum(1 for i in ins if i.startswith('v_readlane'))}, v_writelane {sum(1 for i in ins if i.startswith('v_writelane'))}, "
                  f"calls {sum(1 for i in ins if i.startswith('s_swappc'))}")
            for what, c in (("loads", ld), ("stores", st)):
                if c:
                    print(f"    {what} by stack offset: " + ", ".join(f"{o}: {n}" for o, n in sorted(c.items())))
            if depth >= 1:
                loops_ld += sum(ld.values()); loops_wait += waits
        print(f"  in loops (depth >= 1): {loops_ld} scratch loads, {loops_wait} vmcnt(0) waits")
        print("  whole body: " + ", ".join(f"{k} {v}" for k, v in spill_figures(raw).items()))


def function_table(lines):
    print("functions of the translation unit: " + " / ".join(spill_figures([]).keys()))
    for ln in lines:
        m = re.match(r"^(_ZN\d+mpcx\w*?\d+\w+?E\S*):", ln)
        if not m:
            continue
        f = spill_figures(function_lines(lines, m.group(1))[1:])
        if any(f.values()):
            print(f"  {short_name(m.group(1))}: " + " / ".join(str(v) for v in f.values()))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--src", default=os.path.join(ROOT, "mpconstellation_amd", "csrc", "solve.hip"))
    ap.add_argument("--asm", help="read this assembly file instead of compiling")
    ap.add_argument("--keep", help="keep the compiled assembly here")
    ap.add_argument("--func", action="append", default=[], help="whole-function instruction counts of this function")
    ap.add_argument("--kernel", action="append", default=[], help="register / spill / scratch / LDS figures of this kernel")
    ap.add_argument("--driver", action="append", default=[], help="spill traffic of this function's body (kernel or device function) per loop depth, and spill figures of every function")
    args = ap.parse_args()
    if args.asm:
        path = args.asm
    else:
        path = args.keep or os.path.join(tempfile.mkdtemp(), "solve.s")
        compile_asm(args.src, path)
    text = open(path).read()
    lines = text.splitlines()
    if args.func or args.kernel or args.driver:
        for name in args.driver:
            driver_census(lines, name)
        if args.driver:
            function_table(lines)
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
