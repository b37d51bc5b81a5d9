"""Compare the device code of two source trees kernel by kernel (developer tool, needs no GPU):

    python tools/isa_diff.py OLD_TREE [NEW_TREE]        (NEW_TREE: this tree)

Every source in each tree's own build.SOURCES is compiled to gfx950 assembly with that tree's FLAGS / FILE_FLAGS
(tools/kernel_regs.py: device_asm).  Per kernel symbol the instruction stream (label .. .Lfunc_end, comments and blank lines dropped,
function-numbered local labels .LBB<n>_ rewritten to .LBB_) and the kernel-level amdhsa.kernels metadata are compared; a kernel may
have moved to another file.  Prints the symbols only one tree has, `identical` or `DIFF` per kernel, one line per source file and the
totals.  Exit status 1 if any kernel differs or is missing.  For refactors that must leave the device code alone."""
import os, re, sys
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from kernel_regs import device_asm, kernel_meta, load_build


def kernel_bodies(asm, names):
    """{kernel: [instruction / directive lines]} for the kernel symbols `names` of one assembly listing."""
    out, cur = {}, None
    for line in asm.splitlines():
        s = line.split(";", 1)[0].rstrip()
        if cur is None:
            if s.endswith(":") and s[:-1] in names:
                cur = out.setdefault(s[:-1], [])
            continue
        if s.startswith(".Lfunc_end"):
            cur = None
        elif s.strip():
            cur.append(re.sub(r"\.LBB\d+_", ".LBB_", " ".join(s.split())))
    return out


def tree_kernels(root):
    """{kernel: (source file, body lines, metadata dict)} over every source of the tree, and {source file: kernel count}."""
    b = load_build(root)
    with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as pool:
        asms = list(pool.map(lambda s: device_asm(root, os.path.join(b.CSRC, s)), b.SOURCES))
    kernels, per_file = {}, {}
    for src, asm in zip(b.SOURCES, asms):
        meta = kernel_meta(asm, fields=None)
        bodies = kernel_bodies(asm, set(meta))
        per_file[src] = len(meta)
        for name, m in meta.items():
            if name in kernels:
                raise RuntimeError(f"kernel {name} is built by both {kernels[name][0]} and {src}")
            kernels[name] = (src, bodies.get(name, []), m)
    return kernels, per_file


def main():
    old_root = os.path.abspath(sys.argv[1])
    new_root = os.path.abspath(sys.argv[2]) if len(sys.argv) > 2 else os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    old, old_files = tree_kernels(old_root)
    new, new_files = tree_kernels(new_root)
    for name in sorted(set(old) - set(new)):
        print(f"only in OLD ({old[name][0]}): {name}")
    for name in sorted(set(new) - set(old)):
        print(f"only in NEW ({new[name][0]}): {name}")
    same, diff = {}, {}
    for name in sorted(set(old) & set(new), key=lambda n: (new[n][0], n)):
        (osrc, obody, ometa), (nsrc, nbody, nmeta) = old[name], new[name]
        where = nsrc if osrc == nsrc else f"{osrc} -> {nsrc}"
        if obody == nbody and ometa == nmeta:
            same[nsrc] = same.get(nsrc, 0) + 1
            print(f"identical  {where}: {name}")
        else:
            diff[nsrc] = diff.get(nsrc, 0) + 1
            changed = ", ".join(f"{k} {ometa.get(k)} -> {nmeta.get(k)}" for k in sorted(set(ometa) | set(nmeta)) if ometa.get(k) != nmeta.get(k))
            print(f"DIFF       {where}: {name}: instructions {len(obody)} -> {len(nbody)}" + (f"; {changed}" if changed else ""))
    print("== per source file: OLD tree")
    for src, n in old_files.items():
        print(f"{src:28s} {n:4d} kernels")
    print("== per source file: NEW tree")
    for src, n in new_files.items():
        print(f"{src:28s} {n:4d} kernels  {same.get(src, 0):4d} identical  {diff.get(src, 0):4d} DIFF")
    missing = len(set(old) ^ set(new))
    print(f"== total: OLD {len(old)} kernels, NEW {len(new)} kernels: {sum(same.values())} identical, {sum(diff.values())} DIFF, "
          f"{missing} in one tree only")
    return 1 if diff or missing else 0


if __name__ == "__main__":
    sys.exit(main())
