"""Is the device code of two trees the same? For a change that touches host code only.

usage: python scripts/device_code_diff.py PARENT_TREE NEW_TREE file.hip [file.hip ...]   (no GPU needed)

Each file's device side is compiled alone with the library's flags (wam_amd/build.py), both trees in
turn at one staging path, because kernels in an anonymous namespace carry a hash of the source path:
  hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -munsafe-fp-atomics --cuda-device-only -c file.hip
The gfx950 code object is unbundled (clang-offload-bundler) and compared: byte for byte; then the
names of the function and object symbols (llvm-readelf -sW; kernels, kernel descriptors), the amdhsa.kernels metadata entries (llvm-readelf --notes:
registers, LDS, scratch, kernarg layout) as a set, and the disassembly (llvm-objdump -d) function by
function, whatever order the functions stand in. Dropped from a function's listing: each
instruction's address and the alignment padding behind the symbol's own size. A pc-relative address
(s_getpc_b64, then s_add_u32 with a 32-bit literal) moves with the function, so its literal is
replaced by the symbol + offset it resolves to. Mnemonics, operands, encodings and symbol-relative
branch targets are kept. Exit status 1 when any function's code or metadata differs."""
import bisect
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
BIN = os.path.join(ROCM, "lib", "llvm", "bin")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-munsafe-fp-atomics", "--cuda-device-only", "-c"]


def tool(name, *args):
    return subprocess.run([os.path.join(BIN, name)] + list(args), check=True, stdout=subprocess.PIPE).stdout.decode()


def code_objects(tree, files, stage, side):
    """{file: path of its gfx950 ELF}, compiled under stage/tree"""
    root = os.path.join(stage, "tree")
    shutil.rmtree(root, ignore_errors=True)
    shutil.copytree(os.path.join(tree, "wam_amd", "csrc"), os.path.join(root, "wam_amd", "csrc"))
    shutil.copytree(os.path.join(tree, "include"), os.path.join(root, "include"))
    os.makedirs(os.path.join(stage, side))
    jobs, out = [], {}
    for f in files:
        obj = os.path.join(stage, side, f + ".o")
        out[f] = obj[:-2] + ".elf"
        jobs.append((f, obj, subprocess.Popen(["hipcc"] + FLAGS + [f, "-o", obj],
                                              cwd=os.path.join(root, "wam_amd", "csrc"))))
    for f, obj, j in jobs:
        if j.wait():
            sys.exit("hipcc failed on %s of %s" % (f, tree))
        tool("clang-offload-bundler", "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
             "--input=" + obj, "--output=" + out[f])
    return out


def symtab(elf):
    """sorted (address, name, size) of the defined function and object symbols"""
    syms = []
    for line in tool("llvm-readelf", "-sW", elf).splitlines():
        f = line.split()
        if len(f) >= 8 and f[0].rstrip(":").isdigit() and f[3] in ("OBJECT", "FUNC") and f[6] != "UND":
            syms.append((int(f[1], 16), f[7], int(f[2])))
    return sorted(syms)


def functions(elf, syms):
    """{function: normalised listing}, the number of pc-relative addresses resolved"""
    size = {n: z for _, n, z in syms}
    out, name, pc, npc, end = {}, None, None, 0, 0
    for line in tool("llvm-objdump", "-d", elf).splitlines():
        s = line.strip()
        m = re.match(r"^([0-9a-f]+) <(.+)>:$", s)
        if m:
            name = m.group(2)
            out[name] = []
            end = int(m.group(1), 16) + size[name]
            continue
        m = re.search(r"// ([0-9A-Fa-f]+):", s)
        if name is None or not m:
            continue
        addr = int(m.group(1), 16)
        if addr >= end:  # alignment padding behind the symbol's own size
            continue
        s = re.sub(r"// [0-9A-Fa-f]+:", "//", s)
        if pc is not None and s.startswith("s_add_u32") and re.search(r"// 80[0-9A-F]{2}FF[0-9A-F]{2} [0-9A-F]{8}$", s):
            lit = int(s[-8:], 16)
            lit -= (lit >> 31) << 32
            i = bisect.bisect_right(syms, (pc + lit, "\xff", 0)) - 1
            s = re.sub(r"0x[0-9a-f]+ +// (\S+) \S+$", r"<pcrel> // \1 ", s) + "%s+0x%x" % (syms[i][1], pc + lit - syms[i][0])
            npc += 1
        pc = addr + 4 if s.startswith("s_getpc_b64") else None
        out[name].append(s)
    return out, npc


def metadata(elf):
    txt = tool("llvm-readelf", "--notes", elf)
    body, _, tail = txt[txt.index("amdhsa.kernels:"):].partition("\namdhsa.")
    return sorted(re.split(r"\n  - ", body)[1:]), tail


def main():
    parent, new, files = sys.argv[1], sys.argv[2], sys.argv[3:]
    stage = tempfile.mkdtemp(prefix="devcode.")
    a = code_objects(parent, files, stage, "parent")
    b = code_objects(new, files, stage, "new")
    bad = 0
    for f in files:
        if open(a[f], "rb").read() == open(b[f], "rb").read():
            print("%s: code objects byte-identical" % f)
            continue
        sa, sb = symtab(a[f]), symtab(b[f])
        fa, na = functions(a[f], sa)
        fb, nb = functions(b[f], sb)
        # __hip_cuid_<hash of the source text>: the one symbol whose name follows the host code
        names = [sorted(n for _, n, _ in s if not n.startswith("__hip_cuid_")) for s in (sa, sb)]
        names = names[0] == names[1]
        differ = sorted(set(fa) ^ set(fb)) + sorted(k for k in set(fa) & set(fb) if fa[k] != fb[k])
        ma, mb = metadata(a[f]), metadata(b[f])
        order = [n for _, n, _ in sa if n in fa] == [n for _, n, _ in sb if n in fb]
        print("%s: code objects differ; %d symbols, lists %s; %d functions (%d of them kernels), %d instructions, "
              "%d / %d pc-relative addresses resolved; functions whose code differs: %d; kernel metadata %s; "
              "functions in the same order: %s"
              % (f, len(sa), "equal" if names else "DIFFERENT", len(fa), len(ma[0]), sum(map(len, fa.values())), na, nb,
                 len(differ), "equal" if ma == mb else "DIFFERENT", "yes" if order else "no"))
        for k in differ[:10]:
            print("    ", k)
        bad += bool(differ) or not names or ma != mb
    shutil.rmtree(stage)
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
