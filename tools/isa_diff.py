"""development aid: `python tools/isa_diff.py <old.s> <new.s> [name filter]` — have the kernels of a translation unit moved?

Both files are device assembly of the same source at two commits, made with the flags of build.build_hip plus
`--cuda-device-only -S`:

  hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -fno-gpu-rdc --cuda-device-only -S -I include \\
        dwarf_bench_amd/csrc/radix.hip -o radix.s

The instruction text of every kernel of <old.s> is compared with the kernel of the same DEMANGLED name in <new.s>
(`.LBB<n>_<m>` labels carry the function's index in the file and are normalised, comments are stripped), and the
resources (LDS bytes, scratch bytes, VGPRs) of the kernels that exist only in <new.s> (or match the filter) are printed.
Exit status 1 if a kernel of <old.s> differs or is gone.
"""
import re
import subprocess
import sys


def load(path):
    txt = open(path).read()
    out = {}
    for m in re.finditer(r"^(_Z\w+):[^\n]*\n(.*?)^\.Lfunc_end\d+:", txt, re.S | re.M):
        body = re.sub(r"\.LBB\d+_", ".LBB_", m.group(2))
        out[m.group(1)] = "\n".join(line.split(";")[0].rstrip() for line in body.split("\n"))
    return out, txt


def demangle(names):
    r = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True)
    return dict(zip(names, r.stdout.splitlines()))


def main():
    if len(sys.argv) < 3:
        raise SystemExit(__doc__)
    old, _ = load(sys.argv[1])
    new, new_txt = load(sys.argv[2])
    flt = sys.argv[3] if len(sys.argv) > 3 else None
    names = demangle(sorted(set(old) | set(new)))
    old = {names[k]: v for k, v in old.items()}
    new = {names[k]: v for k, v in new.items()}
    moved = [k for k in old if new.get(k) != old[k]]
    print(f"{len(old)} kernels in {sys.argv[1]}, {len(new)} in {sys.argv[2]}; instruction text differs or kernel gone: {len(moved)}")
    for k in moved:
        print("  DIFF" if k in new else "  GONE", k)
    for m in re.finditer(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", new_txt, re.S):
        name = names.get(m.group(1), m.group(1))
        if (flt and flt in name) or (not flt and name not in old):
            field = lambda k: re.search(rf"\.amdhsa_{k}\s+(\S+)", m.group(2)).group(1)  # noqa: E731
            short = name.replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0]
            print(f"  {short[:60]:60s} lds {field('group_segment_fixed_size'):>6s}  scratch "
                  f"{field('private_segment_fixed_size'):>3s}  vgprs {field('next_free_vgpr'):>3s}")
    return 1 if moved else 0


if __name__ == "__main__":
    sys.exit(main())
