"""Are the kernels of two builds the same device code?  (development aid; profiles/abi_split.txt)

    hipcc <flags of gpras_amd/_build.py> -S --cuda-device-only -o old/<unit>.s <old tree>/gpras_amd/csrc/<unit>.hip   (every unit)
    hipcc ...                                                    -o new/<unit>.s gpras_amd/csrc/<unit>.hip
    python tools/isa_compare.py old new [--rename 'OLD TEXT=NEW TEXT' ...]

Kernels are matched by demangled name; each --rename replaces OLD TEXT by NEW TEXT in the old build's demangled names first (a
template parameter list that shrank: 'potrf_panel_kernel<2, 2, false>=potrf_panel_kernel<false>', profiles/potrf_retire.txt).  Two kernels are identical when their instruction text is equal after the local labels
(.LBBn_m) are renumbered in order of appearance and the kernel's own mangled name is blanked (internal linkage changes it),
and their .amdhsa_kernel blocks (VGPR / AGPR / SGPR / scratch / LDS figures) are equal."""
import collections
import glob
import os
import re
import subprocess
import sys


def kernels(path):
    """{mangled name: (normalised body, normalised descriptor)} of one assembly file"""
    lines = open(path).read().split("\n")
    names = [l.split()[1] for l in lines if l.strip().startswith(".amdhsa_kernel ")]
    label = {l.split(":")[0]: i for i, l in enumerate(lines) if re.match(r"[A-Za-z_][\w.$]*:", l)}
    desc = {l.split()[1]: i for i, l in enumerate(lines) if l.strip().startswith(".amdhsa_kernel ")}
    out = {}
    for name in names:
        start, d0 = label[name], desc[name]
        end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
        d1 = next(i for i in range(d0, len(lines)) if lines[i].strip() == ".end_amdhsa_kernel")
        labels = {}

        def norm(text):
            text = text.replace(name[2:] if name.startswith("_Z") else name, "KERNEL")
            return re.sub(r"\.LBB\d+_\d+", lambda m: labels.setdefault(m.group(0), ".L%d" % len(labels)), text)

        body = [norm(l.split(";")[0].rstrip()) for l in lines[start + 1:end]]
        body = [l for l in body if l.strip() and (not l.strip().startswith(".") or l.endswith(":"))]  # instructions and labels, no directives
        out[name] = ("\n".join(body), norm("\n".join(l.strip() for l in lines[d0 + 1:d1])))
    return out


def load(directory):
    found = collections.defaultdict(list)  # demangled -> [(unit, mangled, body, descriptor)]
    for path in sorted(glob.glob(os.path.join(directory, "*.s"))):
        ks = kernels(path)
        plain = subprocess.run(["c++filt"], input="\n".join(ks), capture_output=True, text=True).stdout.splitlines() if ks else []
        for (mangled, (body, desc)), name in zip(ks.items(), plain):
            found[name].append((os.path.basename(path)[:-2], mangled, body, desc))
    return found


old, new = load(sys.argv[1]), load(sys.argv[2])
for spec in sys.argv[4::2] if sys.argv[3:4] == ["--rename"] else []:
    a, _, b = spec.partition("=")
    old = {name.replace(a, b): copies for name, copies in old.items()}
same = renamed = 0
bad = []
for name, copies in sorted(old.items()):
    _, mangled, body, desc = copies[0]
    if name not in new:
        bad.append("missing: " + name)
        continue
    for unit, m2, b2, d2 in new[name]:
        if b2 != body or d2 != desc:
            bad.append("differs (%s) in %s: %s" % ("instructions" if b2 != body else "resources", unit, name))
    same += all(b2 == body and d2 == desc for _, _, b2, d2 in new[name])
    if all(m2 != mangled for _, m2, _, _ in new[name]):
        renamed += 1
        print("renamed: %s -> %s" % (mangled, sorted({m2 for _, m2, _, _ in new[name]})))
for name in sorted(set(new) - set(old)):
    bad.append("new kernel: " + name)
multi = {name: [u for u, _, _, _ in c] for name, c in new.items() if len(c) > 1}
print("kernels in the old build: %d   identical in the new build: %d   of those under a new symbol name: %d" % (len(old), same, renamed))
print("kernels held by more than one new unit: %d" % len(multi))
for name, units in sorted(multi.items()):
    print("  %s: %s" % (", ".join(units), name[:150]))
for b in bad:
    print(b)
sys.exit(1 if bad else 0)
