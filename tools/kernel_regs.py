"""Print registers / scratch / LDS of every kernel in a .hip file (developer tool): python tools/kernel_regs.py file.hip [extra flags]"""
import importlib.util, os, re, subprocess, sys


def load_build(root):
    """The build module of the tree at `root`: its SOURCES / FLAGS / FILE_FLAGS are the ones that tree's library is built with."""
    spec = importlib.util.spec_from_file_location("sed_build_" + str(abs(hash(root))), os.path.join(root, "transformer4sed_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def device_asm(root, src, extra=()):
    """gfx950 assembly of one source file, compiled with the flags the library of the tree at `root` builds it with (per file)."""
    b = load_build(root)
    flags = [f for f in b.FLAGS if f != "-fPIC"] + b.FILE_FLAGS.get(os.path.basename(src), []) + ["-I" + os.path.join(root, "include")] + list(extra)
    r = subprocess.run(["/opt/rocm/bin/hipcc", *flags, "-S", "--cuda-device-only", src, "-o", "-"], capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"hipcc failed on {src}:\n{r.stderr}")
    return r.stdout


def kernel_meta(asm, fields=("vgpr_count", "private_segment_fixed_size", "group_segment_fixed_size")):
    """{kernel name: {field: value}} from the amdhsa.kernels metadata of an assembly listing, in listing order.  fields = None: every
    kernel-level field but the symbol names, the nested ones (.args) as the text of their lines."""
    out, cur, in_meta, nested = {}, {}, False, None

    def flush():
        if "name" in cur:
            name = cur.pop("name")
            cur.pop("symbol", None)
            out[name] = {k: v for k, v in cur.items() if fields is None or k in fields}
        cur.clear()

    for line in asm.splitlines():
        if line.startswith("amdhsa.kernels:"):
            in_meta = True
            continue
        if in_meta and not line.startswith(" "):
            break
        if not in_meta:
            continue
        m = re.match(r"  (?:- |  )\.(\w+):\s*(.*)", line)      # a kernel's own fields: "  - .first:" then "    .next:"
        if m:
            if line.startswith("  - "):
                flush()
            nested = m.group(1)
            cur[nested] = m.group(2)
        elif nested is not None:
            cur[nested] += " | " + line.strip()
    flush()
    return out


if __name__ == "__main__":
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for name, k in kernel_meta(device_asm(root, sys.argv[1], sys.argv[2:])).items():
        if "vgpr_count" in k:
            print("%-70s vgpr %4s scratch %5s lds %6s" % (name[:70], k.get("vgpr_count"), k.get("private_segment_fixed_size"),
                                                          k.get("group_segment_fixed_size")))
