#!/usr/bin/env python3
"""Code size of every device function in a hipcc object or shared library:
extracts the gfx950 code object from the offload bundle in .hip_fatbin and
lists symbol sizes (llvm-readelf). Build tooling (I-cache footprint check).

  python tools/kernel_sizes.py handel_amd/_build/bn256_verify.o
  python tools/kernel_sizes.py --digest handel_amd/_build/libhandel_gpu.so

--digest lists every function's size and the SHA-256 of its bytes, so a
refactor can show that a kernel's machine code did not move (diff two runs).
--digest-masked is the same with PC-relative address literals masked
(masked_digests): for a refactor that moves functions between units, where
each unit's code object has its own copy of a table at another distance.
"""

import struct
import subprocess
import sys
import tempfile

LLVM = "/opt/rocm/lib/llvm/bin/"


def bundles(path):
    data = open(path, "rb").read()
    magic = b"__CLANG_OFFLOAD_BUNDLE__"
    pos = 0
    while True:
        i = data.find(magic, pos)
        if i < 0:
            return
        n = struct.unpack_from("<Q", data, i + 24)[0]
        off = i + 32
        for _ in range(n):
            o, sz, tl = struct.unpack_from("<QQQ", data, off)
            triple = data[off + 24:off + 24 + tl].decode()
            off += 24 + tl
            if "gfx" in triple and sz:
                yield triple, data[i + o:i + o + sz]
        pos = i + 1


def resources(path):
    """{kernel symbol: {"vgpr", "vgpr_spill", "sgpr_spill", "lds", "scratch"}} from
    the gfx950 code objects' metadata notes (llvm-readelf --notes)."""
    import re

    out = {}
    for triple, blob in bundles(path):
        if "gfx950" not in triple:
            continue
        with tempfile.NamedTemporaryFile(suffix=".co") as f:
            f.write(blob)
            f.flush()
            notes = subprocess.run([LLVM + "llvm-readelf", "--notes", f.name], capture_output=True, text=True).stdout
        for b in notes.split("- .agpr_count")[1:]:
            def g(k):
                m = re.search(r"\." + k + r":\s+(\S+)", b)
                return int(m.group(1)) if m else None
            name = re.search(r"\.name:\s+(\S+)", b).group(1)
            out[name] = {"vgpr": g("vgpr_count"), "vgpr_spill": g("vgpr_spill_count"),
                         "sgpr_spill": g("sgpr_spill_count"), "lds": g("group_segment_fixed_size"),
                         "scratch": g("private_segment_fixed_size")}
    return out


def digests(path):
    """{device function symbol: (size, SHA-256 of its bytes)} over the gfx950
    code objects: equal digests in two builds mean equal machine code."""
    import hashlib

    out = {}
    for triple, blob in bundles(path):
        if "gfx950" not in triple:
            continue
        with tempfile.NamedTemporaryFile(suffix=".co") as f:
            f.write(blob)
            f.flush()
            secs = subprocess.run([LLVM + "llvm-readelf", "-SW", f.name], capture_output=True, text=True).stdout
            syms = subprocess.run([LLVM + "llvm-readelf", "-sW", f.name], capture_output=True, text=True).stdout
        where = {}  # section index -> (address, file offset)
        for line in secs.splitlines():
            p = line.replace("[", " ").replace("]", " ").split()
            if len(p) >= 6 and p[0].isdigit() and p[2] in ("PROGBITS", "NOBITS"):
                where[int(p[0])] = (int(p[3], 16), int(p[4], 16))
        for line in syms.splitlines():
            p = line.split()
            if len(p) >= 8 and p[3] == "FUNC" and p[6].isdigit() and int(p[6]) in where:
                addr, off = where[int(p[6])]
                start, size = int(p[1], 16) - addr + off, int(p[2])
                out[p[7]] = (size, hashlib.sha256(blob[start:start + size]).hexdigest())
    return out


def masked_digests(path):
    """{device function symbol: (size, SHA-256)} as digests(), over each
    function's instruction words in order with one thing masked: the 32-bit
    literals of the s_add_u32 / s_addc_u32 pair that follows an s_getpc_b64 on
    the same register pair, i.e. a PC-relative address (a table of the code
    object, another function). That distance changes when a function moves to
    another unit or place; every other word — opcodes, operands, relative
    branch offsets — is hashed as it is, so the digest is position-independent
    and nothing else is."""
    import hashlib
    import re

    ins = re.compile(r"^\s+(\S+)\s*(.*?)\s*// ([0-9A-Fa-f]+): ((?:[0-9A-Fa-f]{8}\s*)+)(?:<\S+>)?$")
    out = {}
    for triple, blob in bundles(path):
        if "gfx950" not in triple:
            continue
        with tempfile.NamedTemporaryFile(suffix=".co") as f:
            f.write(blob)
            f.flush()
            syms = subprocess.run([LLVM + "llvm-readelf", "-sW", f.name], capture_output=True, text=True).stdout
            asm = subprocess.run([LLVM + "llvm-objdump", "-d", f.name], capture_output=True, text=True).stdout
        funcs = sorted({(int(p[1], 16), int(p[2]), p[7]) for p in (l.split() for l in syms.splitlines())
                        if len(p) >= 8 and p[3] == "FUNC" and p[6].isdigit()})  # .dynsym and .symtab list it twice
        rows = []  # (address, mnemonic, operands, words)
        for line in asm.splitlines():
            m = ins.match(line)
            if m:
                rows.append((int(m.group(3), 16), m.group(1), m.group(2), m.group(4).split()))
        i = 0
        for start, size, name in funcs:
            while i < len(rows) and rows[i][0] < start:
                i += 1
            h, nbytes, pair, left = hashlib.sha256(), 0, None, 0
            while i < len(rows) and rows[i][0] < start + size:
                _, op, args, words = rows[i]
                words = list(words)
                a = [x.strip() for x in args.split(",")]
                if op == "s_getpc_b64":
                    lo, hi = re.match(r"s\[(\d+):(\d+)\]", a[0]).groups()
                    pair, left = {"s_add_u32": "s" + lo, "s_addc_u32": "s" + hi}, 2
                elif left:
                    if pair.get(op) == a[0] and a[1] == a[0] and len(words) == 2:
                        words[1] = "PCRELLIT"
                        del pair[op]
                    left -= 1
                h.update(" ".join(words).encode() + b"\n")
                nbytes += 4 * len(words)
                i += 1
            if nbytes != size:
                raise SystemExit(f"{name}: disassembled {nbytes} of {size} bytes")
            out[name] = (size, h.hexdigest())
    return out


def main():
    if sys.argv[1] in ("--digest", "--digest-masked"):  # one line per function: size, SHA-256, symbol
        fn = digests if sys.argv[1] == "--digest" else masked_digests
        for name, (size, sha) in sorted(fn(sys.argv[2]).items()):
            print(f"{size:8d}  {sha}  {name}")
        return
    for triple, blob in bundles(sys.argv[1]):
        with tempfile.NamedTemporaryFile(suffix=".co") as f:
            f.write(blob)
            f.flush()
            out = subprocess.run([LLVM + "llvm-readelf", "-sW", f.name], capture_output=True, text=True).stdout
        rows = []
        for line in out.splitlines():
            p = line.split()
            if len(p) >= 8 and p[3] == "FUNC":
                rows.append((int(p[2]), p[7]))
        print(triple, "total FUNC bytes:", sum(r[0] for r in rows))
        for sz, name in sorted(rows, reverse=True)[:12]:
            print(f"{sz:10d}  {name[:100]}")


if __name__ == "__main__":
    main()
