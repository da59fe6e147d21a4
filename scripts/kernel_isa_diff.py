"""Compare the gfx950 device assembly of two csrc/kernels directories, kernel by kernel. CPU only.

    python scripts/kernel_isa_diff.py OLD_KERNELS_DIR NEW_KERNELS_DIR [file.hip ...]

The check behind a refactor that must not change machine code: every named .hip file (default: every .hip file of
either directory) is compiled from both directories with exactly the flags of the package build
(_build.kernel_flags, per-file flags included) plus `--cuda-device-only -S`, the per-compile `__hip_cuid_*` lines
are dropped, and the text is compared per kernel symbol (label to .end_amdhsa_kernel: code and kernel descriptor)
and for whatever lies outside the kernels (device functions, metadata). Prints one row per kernel -- identical or
DIFFERENT, next free VGPR / SGPR, accum offset, scratch and static LDS bytes (old -> new where they differ) -- and
the first differing lines of each kernel that differs. Exit status 0 only if everything is identical.
"""
import argparse
import concurrent.futures as cf
import difflib
import os
import re
import subprocess
import sys
import tempfile
from pathlib import Path

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from distributedvolunteercomputing_amd import _build  # noqa: E402

FIELDS = (("vgpr", ".amdhsa_next_free_vgpr"), ("sgpr", ".amdhsa_next_free_sgpr"), ("accum", ".amdhsa_accum_offset"),
          ("scratch", ".amdhsa_private_segment_fixed_size"), ("lds", ".amdhsa_group_segment_fixed_size"))
OTHER = "(outside kernels)"


def device_asm(kdir: Path, name: str, tmp: Path, tag: str) -> list[str]:
    out = tmp / f"{tag}_{Path(name).stem}.s"
    cmd = [_build._hipcc(), *_build.kernel_flags(name, kdir), "--cuda-device-only", "-S", str(kdir / name), "-o",
           str(out)]
    proc = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if proc.returncode != 0:
        raise RuntimeError(f"{' '.join(cmd)}\n{proc.stdout}")
    return [ln.rstrip() for ln in out.read_text().splitlines() if "__hip_cuid_" not in ln]


def split_kernels(lines: list[str]) -> dict[str, list[str]]:
    """symbol -> its lines, `symbol:` through `.end_amdhsa_kernel`; OTHER -> every line outside those spans."""
    names = [ln.split()[1] for ln in lines if ln.strip().startswith(".amdhsa_kernel ")]
    start = {}
    for i, ln in enumerate(lines):  # the function label, `symbol:` with a trailing comment
        m = re.match(r"(\S+):", ln)
        if m and m.group(1) in names:
            start.setdefault(m.group(1), i)
    parts, taken = {}, [False] * len(lines)
    for name in names:
        i = start[name]
        j = next(k for k in range(i, len(lines)) if lines[k].strip() == f".amdhsa_kernel {name}")
        end = next(k for k in range(j, len(lines)) if lines[k].strip() == ".end_amdhsa_kernel")
        parts[name] = lines[i:end + 1]
        taken[i:end + 1] = [True] * (end + 1 - i)
    parts[OTHER] = [ln for ln, t in zip(lines, taken) if not t]
    return parts


def descriptor(part: list[str]) -> dict[str, str]:
    d = {}
    for ln in part:
        w = ln.split()
        for key, directive in FIELDS:
            if len(w) == 2 and w[0] == directive:
                d[key] = w[1]
    return d


def short(sym: str) -> str:
    if sym == OTHER:
        return sym
    try:  # binutils' c++filt does not know the bf16 mangling (DF16b): demangle with half in its place
        out = subprocess.run(["c++filt", sym.replace("DF16b", "Dh")], stdout=subprocess.PIPE, text=True).stdout.strip()
    except OSError:
        out = ""
    if not out or out.startswith("_Z"):
        out = sym
    elif "Dh" not in sym:
        out = re.sub(r"\bhalf\b", "bf16", out)
    out = re.sub(r"\(.*\)( \[clone.*\])?$", "", out)  # drop the argument list
    return out if len(out) <= 88 else out[:85] + "..."


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("old", type=Path)
    ap.add_argument("new", type=Path)
    ap.add_argument("files", nargs="*", help="kernel sources to compare (default: every .hip of either directory)")
    ap.add_argument("-j", type=int, default=min(8, os.cpu_count() or 4))
    ap.add_argument("--context", type=int, default=12, help="differing lines shown per kernel")
    a = ap.parse_args(argv)
    old, new = a.old.resolve(), a.new.resolve()
    files = a.files or sorted({p.name for d in (old, new) for p in d.glob("*.hip")})
    bad = 0
    with tempfile.TemporaryDirectory() as td, cf.ThreadPoolExecutor(max_workers=max(1, a.j)) as ex:
        jobs = {}
        for f in files:
            if not ((old / f).exists() and (new / f).exists()):
                print(f"{f}: only in {'NEW' if (new / f).exists() else 'OLD'}: DIFFERENT")
                bad += 1
                continue
            jobs[f] = (ex.submit(device_asm, old, f, Path(td), "old"), ex.submit(device_asm, new, f, Path(td), "new"))
        print(f"{'file':<18}{'kernel':<90}{'code':<11}vgpr sgpr accum scratch lds")
        for f, (fo, fn) in jobs.items():
            po, pn = split_kernels(fo.result()), split_kernels(fn.result())
            for sym in list(po) + [s for s in pn if s not in po]:
                lo, ln = po.get(sym), pn.get(sym)
                same = lo == ln
                bad += not same
                do, dn = descriptor(lo or []), descriptor(ln or [])
                cols = " ".join(do.get(k, "-") if do.get(k) == dn.get(k) else f"{do.get(k, '-')}->{dn.get(k, '-')}"
                                for k, _ in FIELDS) if sym != OTHER else ""
                print(f"{f:<18}{short(sym):<90}{'identical' if same else 'DIFFERENT':<11}{cols}")
                if not same:
                    if lo is None or ln is None:
                        print(f"    only in {'NEW' if lo is None else 'OLD'}")
                        continue
                    diff = [d for d in difflib.unified_diff(lo, ln, "old", "new", n=0, lineterm="")][2:]
                    for d in diff[:a.context]:
                        print("    " + d)
    print(f"{'all identical' if not bad else f'{bad} DIFFERENT'} ({len(files)} files)")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
