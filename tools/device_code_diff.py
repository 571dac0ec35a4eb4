#!/usr/bin/env python3
"""Prove that a host-only change left the device code alone -- no GPU needed.

    python tools/device_code_diff.py OLD_CSRC NEW_CSRC [--pool] [--jobs N] [--keep DIR]

Every .hip of build.py's SOURCES is compiled for the device only from both source trees, with build.py's own FLAGS and
EXTRA_FLAGS (imported, so MPREID_ABLATION=1 in the environment selects the ablation flag set exactly as it does for the
build).  Compared, keyed by symbol name:
  * the bytes of every FUNC symbol in .text (offset and size from `llvm-readelf -sW`),
  * each kernel's entry in the AMDGPU metadata note: register counts, LDS, scratch, kernarg size, workgroup size.
Whole files are NOT compared: two device objects of identical kernels differ in their hashes (the source path is in
there), and moving a launch into a helper may reorder implicit template instantiations -- reported, not an error.
Files are compared one by one; --pool compares one table per tree instead, the union of all its files, for a change that
moves kernels between files (each move is listed; a kernel that left one file for another is neither removed nor added).

Each CSRC directory must sit where its `../../include` resolves (a checkout of the parent commit, e.g. from
`git worktree add DIR HEAD`, gives DIR/mp-reid_amd/csrc).  Exit status 1 if a symbol was added, removed or differs.
"""
from __future__ import annotations

import argparse
import importlib.util
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
META_KEYS = (".vgpr_count", ".sgpr_count", ".group_segment_fixed_size", ".private_segment_fixed_size",
             ".kernarg_segment_size", ".max_flat_workgroup_size")


def load_build():
    spec = importlib.util.spec_from_file_location("mpreid_build", os.path.join(REPO, "mp-reid_amd", "mpreid", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def run(cmd):
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError("failed: " + " ".join(cmd) + "\n" + r.stdout + r.stderr)
    return r.stdout


def functions(readelf, obj):
    """{name: bytes} of the FUNC symbols in .text, and their names in address order"""
    text = None   # (section index, address, file offset)
    for line in run([readelf, "-SW", obj]).splitlines():
        m = re.match(r"\s*\[\s*(\d+)\]\s+\.text\s+PROGBITS\s+([0-9a-f]+)\s+([0-9a-f]+)\s+([0-9a-f]+)", line)
        if m:
            text = (int(m.group(1)), int(m.group(2), 16), int(m.group(3), 16))
    if text is None:
        return {}, []
    blob = open(obj, "rb").read()
    syms = []
    for line in run([readelf, "-sW", obj]).splitlines():
        # Num: Value Size Type Bind Vis Ndx Name
        m = re.match(r"\s*\d+:\s+([0-9a-f]+)\s+(\d+)\s+FUNC\s+\S+\s+\S+\s+(\d+)\s+(\S+)", line)
        if m and int(m.group(3)) == text[0]:
            addr, size = int(m.group(1), 16), int(m.group(2))
            off = addr - text[1] + text[2]
            syms.append((addr, m.group(4), blob[off:off + size]))
    syms.sort()
    return {name: code for _, name, code in syms}, [name for _, name, _ in syms]


def kernel_metadata(readelf, obj):
    """{kernel name: {key: value}} from the amdhsa.kernels list of the metadata note (keys at the entry's own indent only:
    the arguments underneath have a .name of their own)"""
    entries, cur, indent, inside = [], None, None, False
    for line in run([readelf, "--notes", obj]).splitlines():
        if re.match(r"\s*amdhsa\.kernels:", line):
            inside = True
            continue
        if not inside:
            continue
        m = re.match(r"(\s*)- (\.\w+):\s*(.*)$", line)
        if m and (indent is None or len(m.group(1)) + 2 == indent):
            indent = len(m.group(1)) + 2
            cur = {m.group(2): m.group(3).strip()}
            entries.append(cur)
            continue
        m = re.match(r"(\s*)(\.?[\w.]+):\s*(.*)$", line)
        if m and indent is not None and len(m.group(1)) < indent - 2:
            inside = False   # the next top-level key of the note (amdhsa.target, amdhsa.version)
            continue
        if m and cur is not None and len(m.group(1)) == indent:
            cur[m.group(2)] = m.group(3).strip()
    return {e[".name"].strip("'\""): {k: e.get(k) for k in META_KEYS} for e in entries if ".name" in e}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("old_csrc")
    ap.add_argument("new_csrc")
    ap.add_argument("--jobs", type=int, default=4)
    ap.add_argument("--keep", help="keep the device objects in this directory")
    ap.add_argument("--pool", action="store_true",
                    help="compare by symbol over ALL files of each tree (a kernel that moved to another file is compared there)")
    args = ap.parse_args()
    b = load_build()
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    readelf = os.environ.get("LLVM_READELF", "/opt/rocm/lib/llvm/bin/llvm-readelf")
    work = args.keep or tempfile.mkdtemp(prefix="device_code_diff_")
    hips = [s for s in b.SOURCES if s.endswith(".hip")]
    new_files = [s for s in hips if not os.path.exists(os.path.join(args.old_csrc, s))]
    if args.pool:
        # every file of each tree: a kernel is compared wherever it lives now
        sources = {"old": [s for s in hips if s not in new_files], "new": hips}
        for s in new_files:
            print("%-16s only in the new tree: pooled" % s, flush=True)
    else:
        # a source the old tree does not have yet is a NEW file: named, not compared (its kernels cannot change an old one)
        sources = {"old": [s for s in hips if s not in new_files]}
        sources["new"] = sources["old"]
        for s in new_files:
            print("%-16s only in the new tree: not compared" % s, flush=True)
    jobs = []
    for tag, csrc in (("old", args.old_csrc), ("new", args.new_csrc)):
        os.makedirs(os.path.join(work, tag), exist_ok=True)
        for src in sources[tag]:
            obj = os.path.join(work, tag, src[:-4] + ".o")
            jobs.append([hipcc] + b.FLAGS + b.EXTRA_FLAGS.get(src, []) +
                        ["--cuda-device-only", "--no-gpu-bundle-output", "-c", os.path.join(csrc, src), "-o", obj])
    print("flags: " + " ".join(b.FLAGS) + "  extra: " + repr(b.EXTRA_FLAGS), flush=True)
    with ThreadPoolExecutor(max_workers=max(1, args.jobs)) as ex:
        list(ex.map(run, jobs))

    def pooled(tag, srcs):
        """functions and metadata of all files of one tree in one table each, keyed by symbol (a symbol that two files
        of a tree define -- one template instance used in both -- is keyed 'symbol [file]' in the later one)"""
        f_all, m_all, home = {}, {}, {}
        for src in srcs:
            obj = os.path.join(work, tag, src[:-4] + ".o")
            f, _ = functions(readelf, obj)
            for table, part in ((f_all, f), (m_all, kernel_metadata(readelf, obj))):
                for k, v in part.items():
                    table[k + " [" + src + "]" if k in table else k] = v
            for k in f:
                home.setdefault(k, src)
        return f_all, m_all, home

    bad = 0
    tot_funcs = tot_kernels = 0
    if args.pool:
        pool_o, pool_n = pooled("old", sources["old"]), pooled("new", sources["new"])
        moved = {}
        for k in set(pool_o[2]) & set(pool_n[2]):
            if pool_o[2][k] != pool_n[2][k]:
                moved.setdefault((pool_o[2][k], pool_n[2][k]), []).append(k)
        for (src_o, src_n), names in sorted(moved.items()):
            print("moved %s -> %s: %d functions" % (src_o, src_n, len(names)))
        units = [("all files", pool_o[0], [], pool_n[0], [], pool_o[1], pool_n[1])]
    else:
        units = []
        for src in sources["new"]:
            o, n = (os.path.join(work, t, src[:-4] + ".o") for t in ("old", "new"))
            units.append((src,) + functions(readelf, o) + functions(readelf, n) +
                         (kernel_metadata(readelf, o), kernel_metadata(readelf, n)))
    for src, fo, order_o, fn, order_n, mo, mn in units:
        removed = sorted((set(fo) - set(fn)) | (set(mo) - set(mn)))
        added = sorted((set(fn) - set(fo)) | (set(mn) - set(mo)))
        code_diff = sorted(k for k in set(fo) & set(fn) if fo[k] != fn[k])
        meta_diff = sorted(k for k in set(mo) & set(mn) if mo[k] != mn[k])
        common = set(fo) & set(fn)
        reordered = [k for k in order_o if k in common] != [k for k in order_n if k in common]
        tot_funcs += len(fn)
        tot_kernels += len(mn)
        ok = not (removed or added or code_diff or meta_diff)
        print("%-16s %4d functions (%7d bytes), %4d kernels: %s%s" % (
            src, len(fn), sum(len(v) for v in fn.values()), len(mn), "identical" if ok else "DIFFERENT",
            ", symbol order changed" if reordered else ""))
        for k in removed:
            print("    removed: " + k)
        for k in added:
            print("    added:   " + k)
        for k in code_diff:
            print("    code differs (%d -> %d bytes): %s" % (len(fo[k]), len(fn[k]), k))
        for k in meta_diff:
            print("    metadata differs: %s\n        old %r\n        new %r" % (k, mo[k], mn[k]))
        bad += not ok
    print("%d files, %d functions, %d kernels: %s" % (
        len(sources["new"]), tot_funcs, tot_kernels,
        "no kernel added, removed or different" if not bad else "%d file(s) DIFFER" % bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
