#!/usr/bin/env python3
"""Compare the gfx950 device code of two builds: codeobj_diff.py OLD NEW, each a bundled device object
(hipcc FLAGS SCHED --cuda-device-only -c dpt_kernels.hip) or a libdpt.so.  Prints every symbol that
differs; exits 1 unless both hold the same function / kernel-descriptor symbols, every function's bytes
are equal and a descriptor (.kd) differs at most in kernel_code_entry_byte_offset (bytes 16..23: where
the kernel sits in the ELF).  __hip_cuid_* (a hash of the source) is ignored."""
import struct
import sys

MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def code_objects(blob):
    """the amdgcn ELF images of every uncompressed offload bundle in the file"""
    at = blob.find(MAGIC)
    while at >= 0:
        (n,) = struct.unpack_from("<Q", blob, at + len(MAGIC))
        q = at + len(MAGIC) + 8
        for _ in range(n):
            off, size, tl = struct.unpack_from("<QQQ", blob, q)
            triple = blob[q + 24:q + 24 + tl].decode()
            q += 24 + tl
            if "amdgcn" in triple and size:
                yield blob[at + off:at + off + size]
        at = blob.find(MAGIC, q)


def symbols(elf):
    """name -> bytes of every defined FUNC / OBJECT symbol of an ELF64 image"""
    assert elf[:6] == b"\x7fELF\x02\x01", "not a little-endian ELF64 image"
    shoff, = struct.unpack_from("<Q", elf, 0x28)
    shentsize, shnum = struct.unpack_from("<HH", elf, 0x3A)
    # (type, addr, offset, size, link, entsize) per section
    sec = [struct.unpack_from("<4xI8xQQQI4x8xQ", elf, shoff + k * shentsize) for k in range(shnum)]
    out = {}
    for typ, _, off, size, link, ent in sec:
        if typ != 2:   # SHT_SYMTAB
            continue
        stroff = sec[link][2]
        for s in range(off, off + size, ent):
            name, info, _, shndx, value, ssize = struct.unpack_from("<IBBHQQ", elf, s)
            if (info & 15) not in (1, 2) or shndx == 0 or shndx >= shnum or not ssize:
                continue
            nm = elf[stroff + name:elf.index(b"\0", stroff + name)].decode()
            styp, saddr, soff = sec[shndx][:3]
            pos = soff + value - saddr
            out[nm] = b"" if styp == 8 else elf[pos:pos + ssize]   # (SHT_NOBITS: size only)
    return out


def load(path):
    syms = {}
    with open(path, "rb") as f:
        for elf in code_objects(f.read()):
            syms.update(symbols(elf))
    if not syms:
        sys.exit("%s: no uncompressed amdgcn code object found" % path)
    return {k: v for k, v in syms.items() if not k.startswith("__hip_cuid_")}


def main(old_path, new_path):
    old, new = load(old_path), load(new_path)
    bad = moved = 0
    for nm in sorted(old.keys() | new.keys()):
        a, b = old.get(nm), new.get(nm)
        if a is None or b is None:
            print("%s only: %s" % ("old" if b is None else "new", nm))
            bad += 1
        elif a != b:
            entry_only = nm.endswith(".kd") and len(a) == len(b) == 64 and a[:16] + a[24:] == b[:16] + b[24:]
            print("%s: %s" % ("entry offset" if entry_only else "DIFFERS (%d / %d bytes)" % (len(a), len(b)), nm))
            moved += entry_only
            bad += not entry_only
    print("%d symbols, %d kernels; %d descriptors differ in the entry offset only, %d other differences"
          % (len(new), sum(k.endswith(".kd") for k in new), moved, bad))
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))
