#!/usr/bin/env python3
"""Compare the gfx950 device code of two builds of the kernel library, kernel by kernel.

    python tools/compare_kernels.py PARENT_BUILD_DIR BRANCH_BUILD_DIR [-v]

A build directory is mrn_amd/csrc/build of a checkout (the *.o of mrn_amd/build.py).  The gfx950 code object of every object
file is unbundled and every kernel is matched BY NAME across the whole directory (a refactor may move a kernel to another unit):
disassembly (instruction text and encoding), kernel descriptor and metadata (VGPR / SGPR / AGPR, LDS, scratch, arguments) are
compared, and a kernel that differs is listed with its code size, registers and scratch on both sides (-v: also the first differing
instructions, and every identical kernel).  Two things that depend on where a kernel sits in its unit and not on the kernel are left
out of the comparison: the literal of a pc-relative address of a constant table, and the alignment padding behind the code.
Exit status 1 when the kernel sets differ or any kernel does.  Uses nothing but ROCm's llvm-objdump and llvm-readelf.
"""
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get("ROCM_LLVM_BIN", "/opt/rocm/llvm/bin")
ARCH = "gfx950"


def run(tool, *args, cwd=None):
    return subprocess.run([os.path.join(LLVM, tool), *args], cwd=cwd, check=True, capture_output=True, text=True).stdout


def code_objects(build_dir, tmp):
    """unbundle every object of the directory; -> paths of the device code objects"""
    out = []
    for name in sorted(os.listdir(build_dir)):
        if not name.endswith(".o"):
            continue
        work = os.path.join(tmp, name)
        os.makedirs(work)
        os.symlink(os.path.abspath(os.path.join(build_dir, name)), os.path.join(work, name))
        run("llvm-objdump", "--offloading", name, cwd=work)
        out += [os.path.join(work, f) for f in sorted(os.listdir(work)) if f.endswith(ARCH)]
    return out


def sections(text):
    """llvm-objdump -d / -D output -> {symbol: [lines]}"""
    syms, cur = {}, None
    for line in text.splitlines():
        m = re.match(r"^[0-9a-f]{16} <(.+)>:$", line)
        if m:
            cur = syms.setdefault(m.group(1), [])
        elif cur is not None and line.strip() and not line.startswith("Disassembly of section"):
            cur.append(line)
    return syms


def instruction(line):
    """'\\ttext // ADDRESS: ENCODING' -> (text, encoding): the address goes, branch targets are already kernel-relative"""
    text, _, tail = line.partition("//")
    return text.strip(), tail.partition(":")[2].strip()


def position_independent(ins):
    """what depends on where a kernel sits in its unit, not on the kernel: the literal of a pc-relative address (s_getpc_b64, then
    s_add_u32 / s_addc_u32 on that register pair: the distance to the unit's constant tables) and the alignment padding behind the code"""
    out, pair, left = [], None, 0
    for text, enc in ins:
        m = re.match(r"s_getpc_b64 s\[(\d+):(\d+)\]$", text)
        if m:
            pair, left = {"s" + m.group(1), "s" + m.group(2)}, 4
        elif left:
            left -= 1
            m = re.match(r"(s_addc?_u32) (s\d+), (s\d+), (0x[0-9a-f]+|-?\d+)$", text)
            if m and m.group(2) == m.group(3) and m.group(2) in pair and len(enc.split()) == 2:
                text, enc = f"{m.group(1)} {m.group(2)}, {m.group(3)}, <pc-relative>", enc.split()[0] + " ........"
        out.append((text, enc))
    while out and out[-1][0] in ("s_nop 0", "s_code_end", "..."):
        out.pop()
    return out


def kernels_of(build_dir):
    """-> {kernel name: dict(unit, code, kd, meta, size)}"""
    found = {}
    with tempfile.TemporaryDirectory() as tmp:
        for co in code_objects(build_dir, tmp):
            unit = os.path.basename(os.path.dirname(co))
            meta = {}
            for block in re.split(r"\n  - (?=\.)", run("llvm-readelf", "--notes", co).split("amdhsa.kernels:", 1)[-1].split("\namdhsa.target")[0]):
                m = re.search(r"^\s+\.name:\s+(\S+)$", block, re.M)
                if m:
                    meta[m.group(1)] = [l.strip() for l in block.strip().splitlines()]
            code = sections(run("llvm-objdump", "-d", co))
            kds = sections(run("llvm-objdump", "-D", "-j", ".rodata", co))
            for name, lines in meta.items():
                assert name not in found, f"kernel {name} is in two units"
                ins = position_independent([instruction(l) for l in code[name]])
                found[name] = {"unit": unit, "code": ins, "kd": [l.strip() for l in kds[name + ".kd"]], "meta": lines,
                               "size": sum(len(e.split()) * 4 for _, e in ins)}
    return found


def field(k, key):
    for l in k["meta"]:
        if l.startswith(key + ":"):
            return l.split(":", 1)[1].strip()
    return "?"


def describe(k):
    return (f"{k['unit']}: {k['size']} B code, VGPR {field(k, '.vgpr_count')} AGPR {field(k, '.agpr_count')} SGPR {field(k, '.sgpr_count')}, "
            f"LDS {field(k, '.group_segment_fixed_size')}, scratch {field(k, '.private_segment_fixed_size')}, "
            f"spills v{field(k, '.vgpr_spill_count')} s{field(k, '.sgpr_spill_count')}")


def main(argv):
    verbose = "-v" in argv
    dirs = [a for a in argv if a != "-v"]
    if len(dirs) != 2:
        sys.exit(__doc__)
    parent, branch = kernels_of(dirs[0]), kernels_of(dirs[1])
    only_parent, only_branch = sorted(set(parent) - set(branch)), sorted(set(branch) - set(parent))
    names = {n: n for n in set(parent) | set(branch)}      # (mangled: the template arguments tell the instantiations apart)
    exceptions, moved = [], 0
    for name in sorted(set(parent) & set(branch)):
        a, b = parent[name], branch[name]
        moved += a["unit"] != b["unit"]
        what = [part for part in ("code", "kd", "meta") if a[part] != b[part]]
        if what:
            exceptions.append((name, what, a, b))
        elif verbose:
            print(f"identical  {names[name]}  [{b['unit']}]")
    for name in only_parent:
        print(f"ONLY IN PARENT  {names[name]}  [{parent[name]['unit']}]")
    for name in only_branch:
        print(f"ONLY IN BRANCH  {names[name]}  [{branch[name]['unit']}]")
    for name, what, a, b in exceptions:
        print(f"DIFFERS ({', '.join({'code': 'disassembly', 'kd': 'descriptor', 'meta': 'metadata'}[w] for w in what)})  {names[name]}")
        print(f"    parent  {describe(a)}")
        print(f"    branch  {describe(b)}")
        if "code" in what:
            first = next((i for i, (x, y) in enumerate(zip(a["code"], b["code"])) if x != y), min(len(a["code"]), len(b["code"])))
            same_text = [t for t, _ in a["code"]] == [t for t, _ in b["code"]]
            print(f"    {len(a['code'])} vs {len(b['code'])} instructions, first difference at #{first}" + (" (encodings only)" if same_text else ""))
            if verbose:
                for side, k in (("parent", a), ("branch", b)):
                    for t, e in k["code"][first:first + 6]:
                        print(f"      {side}  {t}    ; {e}")
    common = len(set(parent) & set(branch))
    print(f"kernels: {len(parent)} parent / {len(branch)} branch, {common} matched by name ({moved} in another unit), "
          f"identical: {common - len(exceptions)}, exceptions: {len(exceptions)}, only in parent: {len(only_parent)}, only in branch: {len(only_branch)}")
    return 1 if exceptions or only_parent or only_branch else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
