"""Is the device code of the current sources instruction-for-instruction the code of an earlier commit?

    python tools/same_code_as.py [--per-kernel [--allow-removed]] <commit> [source basenames, default: every csrc/*.hip that
                                                                           differs from the commit]

For refactors made without a GPU at hand (macro restructuring, experiment variants behind #ifdef): compiles the named
translation units of <commit> (git archive into a temporary directory) and of the working tree with build.py's flags and
compares the gfx950 disassembly (addresses and encodings stripped). Exit code 1 on any difference.

--per-kernel: the disassembly is split at the kernel symbols and the BODIES are compared as a multiset, whatever they are called
(branch targets are relative, so a body does not depend on its name or position): dropping a template parameter renames every
instantiation and changes none. A kernel whose body finds no partner on the other side is listed by name: removed (old side), added
(new side), or changed (its name is on both lists). Exit code 1 for any changed or added kernel, and for a removed one unless
--allow-removed is given.
"""

import collections
import glob
import importlib.util
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"
SYMBOL = re.compile(r"^[0-9a-f]+ <(.+)>:$")


def _flags():
    spec = importlib.util.spec_from_file_location("pg_build", os.path.join(ROOT, "pytorch-generative_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.HIPCC, [f for f in mod.FLAGS if not f.startswith("-W")]


def _disasm(hipcc, flags, src, workdir, tag):
    obj = os.path.join(workdir, tag + ".o")
    subprocess.run([hipcc, *flags, "-c", src, "-o", obj], check=True, capture_output=True)
    subprocess.run([f"{LLVM}/llvm-objdump", "--offloading", obj], check=True, capture_output=True, cwd=workdir)
    co = glob.glob(obj + ".0.hipv4-amdgcn-amd-amdhsa--gfx950")
    if not co:
        return []  # host-only translation unit (comm.hip)
    text = subprocess.run([f"{LLVM}/llvm-objdump", "-d", "--no-show-raw-insn", co[0]], check=True, capture_output=True,
                          text=True).stdout
    return [ln.split("//")[0].rstrip() for ln in text.splitlines()[3:]]


def kernels(lines):
    """{symbol: body as one string} of a stripped disassembly."""
    out, name = {}, None
    for ln in lines:
        m = SYMBOL.match(ln)
        if m:
            name = m.group(1)
            out[name] = []
        elif name is not None and ln:
            out[name].append(ln)
    return {k: "\n".join(v) for k, v in out.items()}


def compare_kernels(old, new):
    """Pairs the bodies of the two sides off as multisets. Returns (removed, added, changed): names of `old` whose body found no partner,
    names of `new` whose body found none, and the names that are on both of those lists (same kernel, other code)."""
    ko, kn = kernels(old), kernels(new)

    def unmatched(mine, theirs):
        left = collections.Counter(theirs.values())
        out = []
        for name in sorted(mine, key=lambda k: (k not in theirs or theirs[k] != mine[k], k)):  # same name and body pair off first
            if left[mine[name]] > 0:
                left[mine[name]] -= 1
            else:
                out.append(name)
        return out

    gone, new_ = unmatched(ko, kn), unmatched(kn, ko)
    changed = sorted(set(gone) & set(new_))
    return sorted(set(gone) - set(changed)), sorted(set(new_) - set(changed)), changed


def main():
    argv = sys.argv[1:]
    per_kernel, allow_removed = "--per-kernel" in argv, "--allow-removed" in argv
    argv = [a for a in argv if not a.startswith("--")]
    if not argv:
        sys.exit(__doc__)
    commit, names = argv[0], argv[1:]
    hipcc, flags = _flags()
    with tempfile.TemporaryDirectory() as tmp:
        old = os.path.join(tmp, "old")
        os.makedirs(old)
        tar = subprocess.run(["git", "archive", commit, "pytorch-generative_amd/csrc", "include"], cwd=ROOT, check=True,
                             capture_output=True).stdout
        subprocess.run(["tar", "-x", "-C", old], input=tar, check=True)
        if not names:
            changed = subprocess.run(["git", "diff", "--name-only", commit, "--", "pytorch-generative_amd/csrc"], cwd=ROOT,
                                     check=True, capture_output=True, text=True).stdout.split()
            hdr = any(c.endswith(".h") for c in changed)
            names = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(ROOT, "pytorch-generative_amd", "csrc", "*.hip"))
                           if hdr or any(c.endswith(os.path.basename(p)) for c in changed))
        bad = 0
        for n in names:
            a = _disasm(hipcc, flags, os.path.join(old, "pytorch-generative_amd", "csrc", n + ".hip"), tmp, "old_" + n)
            b = _disasm(hipcc, flags, os.path.join(ROOT, "pytorch-generative_amd", "csrc", n + ".hip"), tmp, "new_" + n)
            if not per_kernel:
                same = a == b
                bad += not same
                print(f"{n:20s} {len(b):8d} lines  {'identical' if same else 'DIFFERENT'}")
                continue
            removed, added, changed = compare_kernels(a, b)
            bad += bool(changed or added or (removed and not allow_removed))
            print(f"{n:20s} {len(kernels(b)):4d} kernels  {len(changed)} changed bodies, {len(added)} added, {len(removed)} removed")
            for what, ks in (("changed", changed), ("removed", removed), ("added", added)):
                for k in ks:
                    print(f"    {what:8s} {k}")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
