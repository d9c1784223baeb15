#!/usr/bin/env python3
"""Is the gfx950 device code of two builds the same code?  For moves of kernels between source files.

    scripts/compare_device_code.py OBJDIR_A OBJDIR_B [--lib-a LIB_A --lib-b LIB_B] [--may-differ REGEX]

OBJDIR_*: the build/obj directories of two builds (correlation_amd/build.py, build(force=True)), e.g. of the parent
commit and of the working tree.  Takes the gfx950 code object out of every *.o, and compares per kernel (and per
device function that was not inlined and is a symbol of its own)
  - the instruction text of its disassembly (addresses, encodings and the literals of pc-relative address
    computations aside: those depend on where the kernel lies in its code object),
  - for kernels, the resource fields of the metadata note,
and the sets of kernel names (no kernel may be emitted by two objects of one build).  With --lib-a / --lib-b also the
exported dynamic symbols of the two libraries (the per-translation-unit __hip_cuid_* ids aside).  Prints what differs;
exit status 0 when nothing does (kernels whose name matches --may-differ are reported but do not count).
"""
import argparse
import hashlib
import os
import re
import subprocess
import sys
import tempfile

TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"
FIELDS = [".vgpr_count", ".agpr_count", ".sgpr_count", ".group_segment_fixed_size", ".private_segment_fixed_size",
          ".max_flat_workgroup_size", ".kernarg_segment_size"]


def tool(args, name):
    return os.path.join(args.llvm_bin, name)


def code_object(args, obj, tmp):
    """gfx950 code object of one host object file (None: the object holds no device code)"""
    fat = os.path.join(tmp, os.path.basename(obj) + ".fat")
    co = os.path.join(tmp, os.path.basename(obj) + ".co")
    subprocess.run([tool(args, "llvm-objcopy"), "-O", "binary", "--only-section=.hip_fatbin", obj, fat], check=True)
    if not os.path.exists(fat) or os.path.getsize(fat) == 0:
        return None
    subprocess.run([tool(args, "clang-offload-bundler"), "--unbundle", "--type=o", "--input=" + fat, "--targets=" + TARGET,
                    "--output=" + co], check=True)
    return co


def metadata(args, co):
    """kernel name -> {field: value} from the amdhsa.kernels list of the metadata note"""
    text = subprocess.run([tool(args, "llvm-readelf"), "--notes", co], check=True, capture_output=True, text=True).stdout
    kernels, cur, item_indent, inside = [], None, None, False
    for line in text.split("\n"):
        if line.strip() == "amdhsa.kernels:":
            inside, item_indent = True, None
            continue
        if not inside:
            continue
        m = re.match(r"^(\s*)- (\.\w+):\s*(.*)$", line)
        if m and (item_indent is None or len(m.group(1)) == item_indent):
            item_indent = len(m.group(1))
            cur = {m.group(2): m.group(3).strip()}
            kernels.append(cur)
            continue
        m = re.match(r"^(\s*)(\.\w+):\s*(.*)$", line)
        if m and item_indent is not None and len(m.group(1)) == item_indent + 2:
            cur[m.group(2)] = m.group(3).strip()
        elif item_indent is not None and line.strip() and len(line) - len(line.lstrip()) < item_indent:
            inside = False  # the list is over (amdhsa.target, amdhsa.version)
    return {k[".name"].strip("'\""): {f: k.get(f) for f in FIELDS} for k in kernels}


def disassembly(args, co):
    """symbol of the text section -> (sha256 of the instruction text, instructions): kernels and device functions that
    were not inlined alike"""
    p = subprocess.Popen([tool(args, "llvm-objdump"), "-d", co], stdout=subprocess.PIPE, text=True)
    out, name, h, n, pc_regs, pc_left = {}, None, None, 0, None, 0

    def close():
        if name is not None:
            out[name] = (h.hexdigest(), n)

    for line in p.stdout:
        m = re.match(r"^[0-9a-f]+ <(.+)>:\s*$", line)
        if m:
            close()
            name, h, n, pc_left = m.group(1), hashlib.sha256(), 0, 0
            continue
        if name is None or not line.startswith("\t"):
            continue
        ins = line.split("//")[0].strip()
        if not ins or ins == "...":  # (a run of zero bytes: padding behind the last function)
            continue
        # s_getpc_b64 s[a:b]; s_add_u32 sa, sa, LITERAL; s_addc_u32 sb, sb, LITERAL: the distance to a symbol
        m = re.match(r"^s_getpc_b64 s\[(\d+):(\d+)\]", ins)
        if m:
            pc_regs, pc_left = ("s" + m.group(1), "s" + m.group(2)), 4
        elif pc_left > 0:
            pc_left -= 1
            m = re.match(r"^(s_addc?_u32|s_subb?_u32) (s\d+), (s\d+), (0x[0-9a-f]+|-?\d+)$", ins)
            if m and m.group(2) == m.group(3) and m.group(2) in pc_regs:
                ins = "%s %s, %s, <pc-relative>" % (m.group(1), m.group(2), m.group(3))
        h.update(ins.encode() + b"\n")
        n += 1
    close()
    if p.wait() != 0:
        raise RuntimeError("llvm-objdump failed on " + co)
    return out


def survey(args, objdir):
    """kernel name -> (object file, metadata fields, (hash, instructions)); the kernel names that occur twice; and
    name -> sorted [(hash, instructions)] of the other functions (internal linkage: one copy per object that calls them)"""
    kernels, twice, functions = {}, [], {}
    with tempfile.TemporaryDirectory() as tmp:
        for f in sorted(os.listdir(objdir)):
            if not f.endswith(".o"):
                continue
            co = code_object(args, os.path.join(objdir, f), tmp)
            if co is None:
                continue
            meta = metadata(args, co)
            dis = disassembly(args, co)
            for k, d in dis.items():
                if k not in meta:
                    functions.setdefault(k, []).append(d)
            for k, fields in meta.items():
                if k in kernels:
                    twice.append((k, kernels[k][0], f))
                kernels[k] = (f, fields, dis.get(k))
            os.remove(co)
    return kernels, twice, {k: sorted(v) for k, v in functions.items()}


def exported(args, lib):
    nm = tool(args, "llvm-nm") if os.path.exists(tool(args, "llvm-nm")) else "nm"
    text = subprocess.run([nm, "-D", "--defined-only", lib], check=True, capture_output=True, text=True).stdout
    # (__hip_cuid_<hash>: one per translation unit with device code, named after a hash of its source)
    return {line.split()[-1] for line in text.split("\n") if line.strip() and not line.split()[-1].startswith("__hip_cuid_")}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("objdir_a")
    ap.add_argument("objdir_b")
    ap.add_argument("--lib-a")
    ap.add_argument("--lib-b")
    ap.add_argument("--may-differ", help="regular expression: kernels that are allowed to differ")
    ap.add_argument("--llvm-bin", default=os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin"))
    args = ap.parse_args()
    bad = 0
    a, twice_a, fa_ = survey(args, args.objdir_a)
    b, twice_b, fb_ = survey(args, args.objdir_b)
    print("kernels: %d in A (%d objects), %d in B (%d objects)" %
          (len(a), len({v[0] for v in a.values()}), len(b), len({v[0] for v in b.values()})))
    for side, twice in (("A", twice_a), ("B", twice_b)):
        for k, f1, f2 in twice:
            print("TWICE in %s: %s (%s, %s)" % (side, k, f1, f2))
            bad += 1
    for k in sorted(set(a) - set(b)):
        print("ONLY in A: %s (%s)" % (k, a[k][0]))
        bad += 1
    for k in sorted(set(b) - set(a)):
        print("ONLY in B: %s (%s)" % (k, b[k][0]))
        bad += 1
    allowed = re.compile(args.may_differ) if args.may_differ else None
    same = 0
    for k in sorted(set(a) & set(b)):
        (fa, ma, da), (fb, mb, db) = a[k], b[k]
        what = []
        if da is None or db is None:
            what.append("no disassembly")
        elif da != db:
            what.append("instructions (%d -> %d)" % (da[1], db[1]))
        what += ["%s %s -> %s" % (f, ma[f], mb[f]) for f in FIELDS if ma[f] != mb[f]]
        if not what:
            same += 1
            continue
        ok = allowed is not None and allowed.search(k) is not None
        print("%s: %s [%s -> %s]: %s" % ("differs (allowed)" if ok else "DIFFERS", k, fa, fb, "; ".join(what)))
        bad += 0 if ok else 1
    print("%d kernels identical (instruction text and %s)" % (same, ", ".join(FIELDS)))
    # device functions that are symbols of their own: a change there leaves the calling kernel's text as it was
    for k in sorted(set(fa_) | set(fb_)):
        if fa_.get(k) != fb_.get(k):
            print("DIFFERS: function %s: %s -> %s" % (k, [n for _, n in fa_.get(k, [])] or "absent", [n for _, n in fb_.get(k, [])] or "absent"))
            bad += 1
    print("%d other function symbols in A, %d in B%s" % (len(fa_), len(fb_), "" if fa_ or fb_ else " (everything is inlined into the kernels)"))
    if args.lib_a and args.lib_b:
        ea, eb = exported(args, args.lib_a), exported(args, args.lib_b)
        for s in sorted(ea - eb):
            print("EXPORTED by A only: " + s)
        for s in sorted(eb - ea):
            print("EXPORTED by B only: " + s)
        print("exported dynamic symbols: %d in A, %d in B, %s" % (len(ea), len(eb), "the same set" if ea == eb else "DIFFERENT"))
        bad += 0 if ea == eb else 1
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
