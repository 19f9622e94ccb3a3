"""Identity of the kernels of gfx950 assembly files (hipcc -S --cuda-device-only): per kernel the number of
instructions, a hash of its whole text (label to s_endpgm, comments and .loc / .file lines stripped), a
hash of its .amdhsa_ directive block and the resources that block declares.  Two builds of a kernel with
equal rows are the same machine code.  Diagnostic only.

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -Iinclude -S --cuda-device-only csrc/zc_cfar.hip -o a.s
    python tools/kernel_text.py [--match zc_] a.s b.s ...
"""
import argparse
import hashlib
import re
import subprocess

FIELDS = ("next_free_vgpr", "next_free_sgpr", "group_segment_fixed_size", "private_segment_fixed_size")


def kernels(path):
    text, hsa, cur, blk = {}, {}, None, None
    for line in open(path):
        s = line.split(";")[0].strip()
        m = re.match(r"\.amdhsa_kernel\s+(\S+)", s)
        if m:
            blk = hsa.setdefault(m.group(1), [])
        elif s == ".end_amdhsa_kernel":
            blk = None
        elif blk is not None and s:
            blk.append(s)
        m = re.match(r"(_Z\w+):", s)
        if m and cur is None and "kernel" in m.group(1):
            cur = text.setdefault(m.group(1), [])
        elif cur is not None and s and not s.startswith((".loc", ".file")):
            cur.append(s)
            if s == "s_endpgm":
                cur = None
    return text, hsa


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("files", nargs="+")
    ap.add_argument("--match", default="", help="only kernels whose demangled name contains this")
    ap.add_argument("--renumber", action="store_true",
                    help="hash the text with the function number of local labels (.LBB<fn>_<n>, .Ltmp<n>) and the "
                         "kernel's own symbol replaced: two builds whose kernels differ only in their place in the "
                         "file or in their mangled name then hash alike")
    a = ap.parse_args()
    sha = lambda rows: hashlib.sha1("\n".join(rows).encode()).hexdigest()[:12]   # noqa: E731
    print("| kernel | instructions | text sha1 | .amdhsa_ sha1 | " + " | ".join(FIELDS) + " |")
    print("|---|---|---|---|" + "---|" * len(FIELDS))
    for path in a.files:
        text, hsa = kernels(path)
        for sym, rows in text.items():
            name = subprocess.run(["c++filt", sym], capture_output=True, text=True).stdout.strip()
            name = re.sub(r"^(void )?(\(anonymous namespace\)::)?|\(.*\)$", "", name)
            if a.match not in name:
                continue
            d = dict(r.split(None, 1) for r in hsa[sym])
            n = sum(1 for r in rows if not r.endswith(":") and not r.startswith("."))
            if a.renumber:
                rows = [re.sub(r"\.LBB\d+_", ".LBB_", r).replace(sym, "@self") for r in rows]
            print(f"| `{name}` | {n} | {sha(rows)} | {sha(hsa[sym])} | " +
                  " | ".join(d[".amdhsa_" + f] for f in FIELDS) + " |")


if __name__ == "__main__":
    main()
