#!/usr/bin/env python3
"""Compare the gfx950 kernels of two builds, object by object (CPU only; needs the ROCm LLVM tools, no GPU and no torch).

    tools/isa_compare.py A/csrc/_obj B/csrc/_obj [--rewrite REGEX REPLACEMENT]... [--unit-rewrite UNIT_REGEX REGEX REPLACEMENT]... [--allow REGEX]...

For every *.o of the two directories the gfx950 code object is extracted (llvm-objcopy of .hip_fatbin, clang-offload-bundler --unbundle),
disassembled (llvm-objdump -d) and its metadata note read (llvm-readelf --notes).  Kernels are paired by demangled name; --rewrite (every
unit) and --unit-rewrite (units whose file name matches UNIT_REGEX) are re.sub pairs applied, in the order given, to the names of side A
first - the way to follow a refactor that renamed kernels or added template arguments.  Reported: kernels on one side only, pairs whose
instruction streams differ (PC-relative offsets of globals and the padding between functions are ignored) and pairs whose SGPR / VGPR / AGPR
counts, fixed LDS, scratch or kernarg size differ.  --allow names kernels (after the rewrites) that are expected to differ: they are listed
but do not count.  The exit status is 0 only if nothing else differs.
"""
import argparse
import glob
import os
import re
import shutil
import subprocess
import sys
import tempfile

ARCH = "gfx950"
META = ("sgpr_count", "vgpr_count", "agpr_count", "group_segment_fixed_size", "private_segment_fixed_size", "kernarg_segment_size")


def tool(name):
    for p in (shutil.which(name), "/opt/rocm/llvm/bin/" + name, "/opt/rocm/lib/llvm/bin/" + name):
        if p and os.path.exists(p):
            return p
    sys.exit(f"{name} not found (ROCm LLVM tools required)")


def run(*cmd):
    return subprocess.run(cmd, check=True, capture_output=True, text=True).stdout


def code_object(obj, tmp):
    """The gfx950 code object of a host object file, or None if it has no device code."""
    fat, co = os.path.join(tmp, "fatbin"), os.path.join(tmp, "co")
    for f in (fat, co):
        if os.path.exists(f):
            os.remove(f)
    subprocess.run([tool("llvm-objcopy"), "-O", "binary", "--only-section=.hip_fatbin", obj, fat], check=True, capture_output=True)
    if not os.path.exists(fat) or os.path.getsize(fat) == 0:
        return None
    subprocess.run([tool("clang-offload-bundler"), "--unbundle", "--type=o", f"--targets=hipv4-amdgcn-amd-amdhsa--{ARCH}",
                    f"--input={fat}", f"--output={co}"], check=True, capture_output=True)
    return co if os.path.exists(co) and os.path.getsize(co) else None


# "<address> <mangled>:" opens a function; an instruction line is "\t<mnemonic operands> // <address>: <encoding words> <branch target>"
_LABEL = re.compile(r"^[0-9a-f]+ <([^>]+)>:$")
# s_getpc_b64 s[a:b]; s_add_u32 sa, sa, LITERAL; s_addc_u32 sb, sb, LITERAL: the address of a global as its distance from the instruction.  The
# literals move with the layout of the unit, not with the kernel's code
_GETPC = re.compile(r"^s_getpc_b64 s\[(\d+):(\d+)\]$")
_PCADD = re.compile(r"^(s_addc?_u32) s(\d+), s(\d+), (0x[0-9a-f]+|-?\d+)$")


def functions(co):
    """mangled name -> list of instructions (text without address and encoding; the padding behind a function dropped)."""
    out, cur, pc = {}, None, set()
    for line in run(tool("llvm-objdump"), "-d", co).splitlines():
        m = _LABEL.match(line)
        if m:
            cur, pc = out.setdefault(m.group(1), []), set()
            continue
        ins = " ".join(line.split("//")[0].split())
        if cur is None or not line.startswith("\t") or not ins or ins == "...":
            continue
        g, m = _GETPC.match(ins), _PCADD.match(ins)
        if g:
            pc = {g.group(1), g.group(2)}
        elif m and m.group(2) == m.group(3) and m.group(2) in pc:
            pc.discard(m.group(2))
            ins = f"{m.group(1)} s{m.group(2)}, s{m.group(3)}, <pc-relative>"
        cur.append(ins)
    for body in out.values():
        while body and body[-1] in ("s_nop 0", "s_code_end"):
            body.pop()
    return out


def metadata(co):
    """mangled kernel name -> tuple of META values, from the amdhsa.kernels list of the code object's metadata note."""
    kernels, inside = [], False
    for line in run(tool("llvm-readelf"), "--notes", co).splitlines():
        if re.match(r"^\S", line):
            inside = line.startswith("amdhsa.kernels:")
        m = re.match(r"^  (- | {2})\.(\w+):\s*(.*)$", line)   # the keys of a kernel's own map: "  - .key:" opens it, "    .key:" goes on
        if not inside or not m:
            continue
        if m.group(1) == "- ":
            kernels.append({})
        kernels[-1][m.group(2)] = m.group(3).strip().strip("'")
    return {k["name"]: tuple(k.get(f, "?") for f in META) for k in kernels}


def unit(obj, rewrites, tmp):
    """demangled (and rewritten) kernel name -> (instructions, metadata) of one object file."""
    co = code_object(obj, tmp)
    if co is None:
        return {}
    fn, meta = functions(co), metadata(co)
    names = list(meta)
    dem = subprocess.run([shutil.which("llvm-cxxfilt") or tool("c++filt")], input="\n".join(names), check=True, capture_output=True,
                         text=True).stdout.splitlines()
    out = {}
    for mangled, name in zip(names, dem):
        for rx, to in rewrites:
            name = re.sub(rx, to, name)
        if name in out:
            sys.exit(f"{obj}: two kernels are named {name} after the rewrites")
        out[name] = (fn.get(mangled, []), meta[mangled])
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("a"), ap.add_argument("b")
    ap.add_argument("--rewrite", nargs=2, action="append", default=[], metavar=("REGEX", "REPLACEMENT"))
    ap.add_argument("--unit-rewrite", nargs=3, action="append", default=[], metavar=("UNIT_REGEX", "REGEX", "REPLACEMENT"))
    ap.add_argument("--allow", action="append", default=[], metavar="REGEX")
    ap.add_argument("--verbose", action="store_true", help="print the first differing instructions of every differing pair")
    args = ap.parse_args()
    objs = [sorted(os.path.basename(p) for p in glob.glob(os.path.join(d, "*.o"))) for d in (args.a, args.b)]
    bad = allowed = total = units = 0
    for o in sorted(set(objs[0]) ^ set(objs[1])):
        print(f"{o}: on one side only")
        bad += 1
    with tempfile.TemporaryDirectory() as tmp:
        for o in sorted(set(objs[0]) & set(objs[1])):
            rw = [(rx, to) for u, rx, to in args.unit_rewrite if re.search(u, o)] + [tuple(r) for r in args.rewrite]
            ka, kb = unit(os.path.join(args.a, o), rw, tmp), unit(os.path.join(args.b, o), [], tmp)
            units += bool(ka or kb)
            for name in sorted(set(ka) | set(kb)):
                what = []
                if name not in ka or name not in kb:
                    what.append("only in " + ("A" if name in ka else "B"))
                else:
                    total += 1
                    (ia, ma), (ib, mb) = ka[name], kb[name]
                    if ia != ib:
                        k = next((i for i, (x, y) in enumerate(zip(ia, ib)) if x != y), min(len(ia), len(ib)))
                        what.append(f"instructions differ ({len(ia)} / {len(ib)}, first at {k}" +
                                    (f": {ia[k]} / {ib[k]})" if args.verbose and k < min(len(ia), len(ib)) else ")"))
                    what += [f"{f}: {x} / {y}" for f, x, y in zip(META, ma, mb) if x != y]
                if not what:
                    continue
                ok = any(re.search(rx, name) for rx in args.allow)
                allowed += ok
                bad += not ok
                print(f"{o}: {name}: " + "; ".join(what) + (" (allowed)" if ok else ""))
    print(f"{total} kernel pairs in {units} units with device code; {bad} differences, {allowed} allowed")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
