#!/usr/bin/env python3
"""Compare the gfx950 kernels of two builds of libsgm_hip.so (no GPU needed).

    tools/kernel_diff.py OLD.so NEW.so

The code objects are taken out of both libraries the way tests/test_isa_guards.py does (the
.hip_fatbin section dumped from a copy with objcopy, clang-offload-bundler --unbundle per bundle).
Per kernel symbol it reports presence in both libraries, the metadata fields FIELDS (llvm-readelf
--notes) and a hash of the kernel's `llvm-objdump -d --no-show-raw-insn` body with everything from
`//` to the end of each line removed: branch operands are relative and the comments carry the only
absolute addresses, so a kernel that merely moved to another address compares equal. Prints the
counts and every differing kernel with the differing fields; exit status 1 on any difference.
"""
import hashlib
import os
import re
import shutil
import subprocess
import sys
import tempfile

LLVM = os.environ.get("ROCM_LLVM_BIN", "/opt/rocm/lib/llvm/bin")
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"
FIELDS = (".vgpr_count", ".agpr_count", ".sgpr_count", ".group_segment_fixed_size", ".private_segment_fixed_size",
          ".kernarg_segment_size", ".max_flat_workgroup_size")


def normalise(body):
    """A kernel's disassembly without its address comments, blank lines and `...` lines (the zero
    padding up to the next symbol's alignment, which depends on where the kernel landed)."""
    lines = (re.sub(r"//.*", "", ln).rstrip() for ln in body.splitlines())
    return "\n".join(ln for ln in lines if ln and ln.strip() != "...")


def body_hash(body):
    return hashlib.sha256(normalise(body).encode()).hexdigest()[:16]


def kernel_bodies(asm):
    """{symbol: body text} of every `<symbol>:` block of an llvm-objdump -d listing."""
    out = {}
    heads = list(re.finditer(r"^[0-9a-f]+ <(\S+)>:\n", asm, re.M))
    for i, m in enumerate(heads):
        end = heads[i + 1].start() if i + 1 < len(heads) else len(asm)
        sect = asm.find("\nDisassembly of section", m.end(), end)
        out[m.group(1)] = asm[m.end():sect if sect >= 0 else end]
    return out


def kernel_metadata(notes):
    """{kernel name: {field: value}} from the amdhsa.kernels list of an llvm-readelf --notes text."""
    out = {}
    for lst in re.finditer(r"^( *)amdhsa\.kernels:\s*\n((?:\1 .*\n|\s*\n)*)", notes, re.M):
        text = lst.group(2)
        first = re.search(r"^( *)- \.", text, re.M)
        if not first:
            continue
        ind = first.group(1)
        for entry in re.split(r"^" + ind + r"- (?=\.)", text, flags=re.M)[1:]:
            entry = ind + "  " + entry                      # the first field back at its siblings' indent
            fields = dict(re.findall(r"^" + ind + r"  (\.\w+): +(\S+)\s*$", entry, re.M))
            if ".name" in fields:
                out[fields[".name"]] = {f: fields.get(f) for f in FIELDS}
    return out


def code_objects(lib, tmp):
    """The gfx950 code objects of a library (paths of the unbundled files under tmp)."""
    objcopy = shutil.which("objcopy")
    if not objcopy:
        raise RuntimeError("objcopy not found")
    # objcopy rewrites its input when no output file is given: work on a copy
    copy = os.path.join(tmp, "lib.so")
    shutil.copyfile(lib, copy)
    fat = os.path.join(tmp, "fatbin")
    subprocess.run([objcopy, "--dump-section", f".hip_fatbin={fat}", copy, os.path.join(tmp, "lib_out.so")],
                   check=True, capture_output=True)
    with open(fat, "rb") as fh:
        data = fh.read()
    starts = [m.start() for m in re.finditer(re.escape(MAGIC), data)]
    if not starts:
        raise RuntimeError(f"{lib}: no offload bundle in .hip_fatbin")
    cos = []
    for i, s in enumerate(starts):
        part = os.path.join(tmp, f"b{i}")
        with open(part, "wb") as fh:
            fh.write(data[s:starts[i + 1] if i + 1 < len(starts) else len(data)])
        co = os.path.join(tmp, f"b{i}.co")
        r = subprocess.run([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", f"--input={part}",
                            f"--targets={TARGET}", f"--output={co}"], capture_output=True)
        if r.returncode == 0 and os.path.exists(co) and os.path.getsize(co) > 0:
            cos.append(co)
    return cos


def code_object_kernels(asm, notes):
    """{kernel symbol: {"meta": ..., "hash": ...}} of one code object's disassembly and notes."""
    bodies = kernel_bodies(asm)
    return {name: {"meta": meta, "hash": body_hash(bodies[name]) if name in bodies else None}
            for name, meta in kernel_metadata(notes).items()}


def merge_kernels(out, more, where):
    """Add one code object's kernels to a library's. A kernel that two code objects define (the
    same template instantiated in two sources) would hide one copy behind the other's key: that is
    an error, not something to compare."""
    dup = sorted(set(out) & set(more))
    if dup:
        raise RuntimeError(f"{where}: defined in more than one code object: {', '.join(dup)}")
    out.update(more)


def library_kernels(lib):
    """{kernel symbol: {"meta": {field: value}, "hash": body hash}} of a built library."""
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for co in code_objects(lib, tmp):
            notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co], check=True,
                                   capture_output=True, text=True).stdout
            asm = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", co], check=True,
                                 capture_output=True, text=True).stdout
            merge_kernels(out, code_object_kernels(asm, notes), lib)
    return out


def compare(old, new):
    """[(kernel, [what differs])] over two library_kernels() results, sorted by kernel."""
    diffs = []
    for name in sorted(set(old) | set(new)):
        if name not in new:
            diffs.append((name, ["only in OLD"]))
        elif name not in old:
            diffs.append((name, ["only in NEW"]))
        else:
            what = [f"{f}: {old[name]['meta'].get(f)} -> {new[name]['meta'].get(f)}" for f in FIELDS
                    if old[name]["meta"].get(f) != new[name]["meta"].get(f)]
            if old[name]["hash"] != new[name]["hash"]:
                what.append(f"body: {old[name]['hash']} -> {new[name]['hash']}")
            if what:
                diffs.append((name, what))
    return diffs


def main(argv):
    if len(argv) != 3:
        sys.stderr.write(__doc__)
        return 2
    old, new = library_kernels(argv[1]), library_kernels(argv[2])
    diffs = compare(old, new)
    ocv = sum(1 for k in new if "k_ocv_" in k)
    print(f"kernels: OLD {len(old)}, NEW {len(new)}, in both {len(set(old) & set(new))} "
          f"(k_ocv_*: {ocv} in NEW, others {len(new) - ocv})")
    print(f"fields: {' '.join(FIELDS)} + body hash")
    for name, what in diffs:
        print(f"DIFF {name}")
        for w in what:
            print(f"    {w}")
    print(f"differing kernels: {len(diffs)}")
    return 1 if diffs else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
