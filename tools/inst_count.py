#!/usr/bin/env python3
"""Static instruction counts of the device code, per function and per loop.  Needs hipcc, no GPU.

Compiles translation units of lodestar_amd/csrc to gfx950 assembly with the flags and defines the product build
gives them (lodestar_amd.build.tu_compile_flags: the same list the library is built from) and tallies every
instruction by mnemonic -- whatever mnemonics occur; nothing is looked for by name.

    python tools/inst_count.py k_sig.hip k_hash.hip --functions '_r$' --loops 'k_sig_subgroup2|k_hash_clear2' -o out.json

--functions REGEX   functions to report (searched in the demangled name without its parameter list; default: all)
--loops REGEX       functions whose loops are reported too.  A loop is the span from a label to the last backward
                    branch to it.  Each loop lists its basic blocks (label to label) with their tallies and calls,
                    so a step inside a larger body (the doubling of a double-and-add loop) can be read off.
--src-root DIR      take the sources from DIR/lodestar_amd/csrc (another checkout, e.g. the parent commit) while
                    the flags still come from this checkout's build.py

Per function / loop / block: "total" instructions, "valu" (mnemonics starting with v_), "mnemonics", "calls"
(callee -> call sites, resolved through the SGPR pair the callee's address was formed in) and "with_callees":
total + sum(calls x the callee's own with_callees) -- the instructions one pass executes when every block runs once.
Functions also carry the "NumVgprs" / "ScratchSize" the assembler comments report.
"""
import argparse
import collections
import concurrent.futures
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from lodestar_amd import build as _build  # noqa: E402

CXXFILT = shutil.which("llvm-cxxfilt") or shutil.which("c++filt")

_LABEL = re.compile(r"^([A-Za-z_.$][\w.$]*):")
_INST = re.compile(r"^\s+([a-z][a-z0-9_]*)\b(.*)$")
_BRANCH = re.compile(r"^s_c?branch")
_SYM_LO = re.compile(r"^\s*s(\d+),\s*s\d+,\s*([\w.$]+)@(?:rel32|gotpcrel32)@lo")
_PAIR = re.compile(r"s\[(\d+):\d+\]")


def compile_asm(tu, src_root=None):
    src = os.path.join(src_root or ROOT, "lodestar_amd", "csrc", tu)
    flags = _build.tu_compile_flags(tu)
    if src_root:
        flags = [os.path.join(src_root, "include") if f == os.path.join(ROOT, "include") else f for f in flags]
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "tu.s")
        subprocess.check_call([_build.HIPCC] + flags + ["--cuda-device-only", "-S", src, "-o", out])
        with open(out) as f:
            return f.read().splitlines(), flags


def demangle(names):
    names = list(names)
    if not names:
        return {}
    if CXXFILT:
        out = subprocess.run([CXXFILT], input="\n".join(names) + "\n", capture_output=True, text=True, check=True)
        dem = out.stdout.splitlines()
    else:  # no demangler: the first component of a plain Itanium name (_Z<len><name>...)
        dem = []
        for n in names:
            m = re.match(r"^_Z(\d+)", n)
            dem.append(n[m.end():m.end() + int(m.group(1))] if m else n)
    res = {}
    for n, d in zip(names, dem):
        # drop the parameter list: everything from the first "(" at template depth 0
        depth, cut = 0, len(d)
        for i, ch in enumerate(d):
            if ch == "<":
                depth += 1
            elif ch == ">":
                depth -= 1
            elif ch == "(" and depth == 0:
                cut = i
                break
        d = d[:cut]
        if d.startswith("void "):
            d = d[5:]
        res[n] = d
    return res


def split_functions(lines):
    """{symbol: (first line, last line)} of every function body, and each one's trailing comment block"""
    types = set()
    for ln in lines:
        m = re.match(r"^\s+\.type\s+([\w.$]+),@function", ln)
        if m:
            types.add(m.group(1))
    funcs, cur, start = {}, None, 0
    for i, ln in enumerate(lines):
        m = _LABEL.match(ln)
        if m and m.group(1) in types and cur is None:
            cur, start = m.group(1), i + 1
        elif cur is not None and re.match(r"^\.Lfunc_end\d+:", ln):
            funcs[cur] = (start, i)
            cur = None
    return funcs


def tally(lines, lo, hi, names):
    """Instruction tally of lines[lo:hi] and the calls in it.  `names`: SGPR index -> symbol (carried along)."""
    mn = collections.Counter()
    calls = collections.Counter()
    for ln in lines[lo:hi]:
        ln = ln.split(";", 1)[0]
        m = _INST.match(ln)
        if not m or _LABEL.match(ln):
            continue
        op, rest = m.group(1), m.group(2)
        mn[op] += 1
        s = _SYM_LO.match(rest)
        if s:
            names[int(s.group(1))] = s.group(2)
        elif op == "s_mov_b64":
            p = _PAIR.findall(rest)
            if len(p) == 2 and int(p[1]) in names:
                names[int(p[0])] = names[int(p[1])]
        elif op == "s_load_dwordx2":
            p = _PAIR.findall(rest)  # an address loaded from the GOT slot formed in p[1]
            if len(p) == 2 and int(p[1]) in names:
                names[int(p[0])] = names[int(p[1])]
        elif op == "s_swappc_b64":
            p = _PAIR.findall(rest)
            calls[names.get(int(p[1]), "?") if len(p) == 2 else "?"] += 1
    return mn, calls


def summarize(mn, calls, dem):
    total = sum(mn.values())
    return {"total": total, "valu": sum(v for k, v in mn.items() if k.startswith("v_")),
            "mnemonics": dict(sorted(mn.items(), key=lambda kv: (-kv[1], kv[0]))),
            "calls": {dem.get(k, k): v for k, v in sorted(calls.items())}}


def loops_of(lines, lo, hi):
    """[(header line, end line, label)] of the loops of one function, outermost first"""
    labels = {}
    for i in range(lo, hi):
        m = _LABEL.match(lines[i])
        if m:
            labels[m.group(1)] = i
    ext = {}
    for i in range(lo, hi):
        m = _INST.match(lines[i].split(";", 1)[0])
        if m and _BRANCH.match(m.group(1)):
            t = m.group(2).strip()
            if t in labels and labels[t] <= i:
                ext[t] = max(ext.get(t, 0), i + 1)
    return sorted(((labels[t], e, t) for t, e in ext.items()), key=lambda x: (x[0], -x[1]))


def analyse(tu, fn_re, loop_re, src_root=None):
    lines, flags = compile_asm(tu, src_root)
    funcs = split_functions(lines)
    dem = demangle(funcs)
    per_fn = {}
    names_at = {}
    for sym, (lo, hi) in funcs.items():
        names = {}
        mn, calls = tally(lines, lo, hi, names)
        names_at[sym] = names
        s = summarize(mn, calls, dem)
        s["_calls_sym"] = dict(calls)
        for ln in lines[hi:hi + 80]:
            m = re.match(r"^\s*;\s*(NumVgprs|NumAgprs|ScratchSize|Occupancy):\s*(\d+)", ln)
            if m and m.group(1) not in s:
                s[m.group(1)] = int(m.group(2))
            if re.match(r"^\s+\.type", ln):
                break
        per_fn[sym] = s

    memo = {}

    def with_callees(sym, seen=()):
        if sym not in per_fn or sym in seen:
            return 0
        if sym not in memo:
            memo[sym] = per_fn[sym]["total"] + sum(n * with_callees(c, seen + (sym,))
                                                   for c, n in per_fn[sym]["_calls_sym"].items())
        return memo[sym]

    def expand(total, calls):
        return total + sum(n * with_callees(c) for c, n in calls.items())

    out = {"flags": [os.path.relpath(f, src_root or ROOT) if os.path.isabs(f) and os.path.exists(f) else f for f in flags],
           "functions": {}, "loops": {}}
    for sym, s in per_fn.items():
        name = dem[sym]
        if fn_re is None or fn_re.search(name):
            e = {k: v for k, v in s.items() if not k.startswith("_")}
            e["with_callees"] = with_callees(sym)
            out["functions"][name] = e
        if loop_re is not None and loop_re.search(name):
            lo, hi = funcs[sym]
            res = []
            for (a, b, label) in loops_of(lines, lo, hi):
                # the SGPR -> callee map as it stands at the loop's entry: addresses are formed before the loop
                names = {}
                tally(lines, lo, a, names)
                mn, calls = tally(lines, a, b, dict(names))
                e = summarize(mn, calls, dem)
                e.update(label=label, depth=sum(1 for (x, y, _) in loops_of(lines, lo, hi) if x <= a and b <= y) - 1,
                         with_callees=expand(e["total"], calls))
                cuts = [i for i in range(a, b) if _LABEL.match(lines[i])] + [b]
                blocks = []
                for x, y in zip(cuts, cuts[1:]):
                    bm, bc = tally(lines, x, y, names)
                    if not bm:
                        continue
                    bs = summarize(bm, bc, dem)
                    blocks.append({"label": _LABEL.match(lines[x]).group(1), "total": bs["total"], "valu": bs["valu"],
                                   "calls": bs["calls"], "with_callees": expand(bs["total"], bc),
                                   "mnemonics": bs["mnemonics"]})
                e["blocks"] = blocks
                res.append(e)
            out["loops"][name] = res
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("units", nargs="+", help="translation units of lodestar_amd/csrc, e.g. k_sig.hip")
    ap.add_argument("--functions", default=None)
    ap.add_argument("--loops", default=None)
    ap.add_argument("--src-root", default=None)
    ap.add_argument("-o", "--output", default=None)
    a = ap.parse_args()
    fn_re = re.compile(a.functions) if a.functions else None
    loop_re = re.compile(a.loops) if a.loops else None
    with concurrent.futures.ThreadPoolExecutor(max_workers=min(len(a.units), 8)) as ex:
        done = list(ex.map(lambda tu: analyse(tu, fn_re, loop_re, a.src_root), a.units))
    res = {"arch": _build.ARCH, "units": dict(zip(a.units, done))}
    text = json.dumps(res, indent=1)
    if a.output:
        with open(a.output, "w") as f:
            f.write(text + "\n")
    else:
        print(text)


if __name__ == "__main__":
    main()
