#!/usr/bin/env python3
"""One line per kernel of the assembly that `make asm` leaves in build/asm: name, a hash of its
instruction text, and the register, scratch and LDS figures of its .amdhsa_kernel block.  Two
checkouts whose device code is the same print the same lines, whatever directory they sit in:
comments and anything that carries a path or a source line are dropped before hashing.

usage: scripts/asm_digest.py [dir with *.s]    (last line: kernel count and a hash of all lines)
"""
import hashlib
import pathlib
import re
import sys

FIGURES = ("next_free_vgpr", "accum_offset", "next_free_sgpr", "private_segment_fixed_size",
           "group_segment_fixed_size")
SKIP = re.compile(r"\s*(;|\.file\b|\.loc\b|\.ident\b|\.cfi_|\.section\s+\.debug)")


def body_lines(lines):
    """The instruction text: no comments, no blank lines, nothing with a path in it."""
    for ln in lines:
        if SKIP.match(ln):
            continue
        ln = ln.split(";", 1)[0].strip()
        if ln and "/" not in ln:
            yield " ".join(ln.split())


def kernels(text):
    """(name, body hash, {figure: value}) of every kernel in one .s file."""
    lines = text.splitlines()
    start = {}  # function name -> line after its label
    for i, ln in enumerate(lines):
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", ln)
        if m:
            name, fig = m.group(1), {}
            for d in lines[i + 1:]:
                if ".end_amdhsa_kernel" in d:
                    break
                f = re.match(r"\s*\.amdhsa_(\w+)\s+(\S+)", d)
                if f and f.group(1) in FIGURES:
                    fig[f.group(1)] = f.group(2)
            a = start[name]
            end = next(j for j in range(a, len(lines)) if lines[j].startswith(".Lfunc_end"))
            h = hashlib.sha256("\n".join(body_lines(lines[a:end])).encode()).hexdigest()[:16]
            yield name, h, fig
        elif re.match(r"[A-Za-z_$][\w$.]*:", ln):
            start.setdefault(ln.split(":", 1)[0], i + 1)


def main():
    here = pathlib.Path(__file__).resolve().parent.parent
    d = pathlib.Path(sys.argv[1]) if len(sys.argv) > 1 else here / "distributed-sorting-with-fault-tolerance_amd/build/asm"
    out = []
    for f in sorted(d.glob("*.s")):
        for name, h, fig in kernels(f.read_text()):
            out.append(f"{f.stem} {name} {h} " + " ".join(f"{k}={fig.get(k, '-')}" for k in FIGURES))
    out.sort()
    print("\n".join(out))
    print(f"# {len(out)} kernels {hashlib.sha256(chr(10).join(out).encode()).hexdigest()[:16]}")


if __name__ == "__main__":
    main()
