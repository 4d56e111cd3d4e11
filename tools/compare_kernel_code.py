"""Compare the gfx950 device code of two builds of recmodel_amd/csrc kernel by kernel: the check that a change to the host
side, to the build, or to which kernels are instantiated left every remaining kernel's instructions alone.

usage: python tools/compare_kernel_code.py OBJDIR_A OBJDIR_B [file.o ...]      (default: every .o the two directories share)

Per object: the kernels (symbols with a .kd descriptor) only A has, only B has, and those in both whose disassembly differs
(branch-target comments and trailing alignment padding stripped, so a kernel that merely moved compares equal).  Exit status 1 if any kernel differs or B
has a kernel that A has not; kernels that only A has are listed (a build that drops kernels is what this tool is for)."""
import hashlib
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get("ROCM_LLVM_BIN", "/opt/rocm/llvm/bin")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"


def run(*cmd, **kw):
    return subprocess.run(cmd, capture_output=True, text=True, check=True, **kw).stdout


def kernels(obj):
    """{mangled kernel name: digest of its instruction text} of the gfx950 code object bundled in a host object file."""
    if ".hip_fatbin" not in run(f"{LLVM}/llvm-readelf", "-S", "--wide", obj):
        return {}                                                # host code only
    with tempfile.TemporaryDirectory() as td:
        fatbin, code = os.path.join(td, "fatbin"), os.path.join(td, "gfx950.co")
        run(f"{LLVM}/llvm-objcopy", f"--dump-section=.hip_fatbin={fatbin}", obj, os.path.join(td, "rest.o"))
        run(f"{LLVM}/clang-offload-bundler", "--type=o", f"--targets={TARGET}", f"--input={fatbin}", f"--output={code}", "--unbundle")
        if not os.path.getsize(code):
            return {}
        listing = run(f"{LLVM}/llvm-objdump", "-d", "--no-show-raw-insn", "--no-leading-addr", code)
        symbols = run(f"{LLVM}/llvm-readelf", "-s", "--wide", code)
    descriptors = {line.split()[-1][:-3] for line in symbols.splitlines() if line.rstrip().endswith(".kd")}
    bodies, name = {}, None
    for line in listing.splitlines():
        head = re.match(r"^[0-9a-f]* ?<(.+)>:$", line)
        if head:
            name = head.group(1)
            bodies[name] = []
        elif name:
            bodies[name].append(re.sub(r"\s*//.*$", "", line).strip())
    # (the zero padding up to the next symbol's alignment, printed as "...", depends on what follows the kernel: not its code)
    return {k: hashlib.sha1("\n".join(line for line in v if line and line != "...").encode()).hexdigest()
            for k, v in bodies.items() if k in descriptors}


def demangled(names):
    return run("c++filt", input="\n".join(names)).splitlines() if names else []


def main(argv):
    if len(argv) < 3:
        sys.exit(__doc__)
    dir_a, dir_b = argv[1], argv[2]
    objects = argv[3:] or sorted(o for o in os.listdir(dir_a) if o.endswith(".o") and os.path.exists(os.path.join(dir_b, o)))
    bad = total_a = total_b = 0
    for o in objects:
        ka, kb = kernels(os.path.join(dir_a, o)), kernels(os.path.join(dir_b, o))
        only_a, only_b = sorted(set(ka) - set(kb)), sorted(set(kb) - set(ka))
        differ = sorted(k for k in set(ka) & set(kb) if ka[k] != kb[k])
        total_a, total_b, bad = total_a + len(ka), total_b + len(kb), bad + len(only_b) + len(differ)
        print(f"{o}: {len(ka)} kernels in A, {len(kb)} in B; only A {len(only_a)}, only B {len(only_b)}, same name different code {len(differ)}")
        for title, names in (("only in A", only_a), ("only in B", only_b), ("DIFFERENT CODE", differ)):
            for line in demangled(names):
                print(f"  {title}: {line}")
    print(f"total: {total_a} kernels in A, {total_b} in B; {bad} kernels new or changed in B")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
