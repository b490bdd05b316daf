#!/usr/bin/env python3
"""Compare the gfx950 kernels of two builds, kernel by kernel.

    python scripts/kernel_isa_digest.py <a> <b>

Each argument is an object file (.o), the library (.so) or a device-only object.  The
gfx950 code objects are taken out of the file's offload bundles (as scripts/co_meta.sh
does for one object; a library holds one bundle per unit), disassembled with the ROCm
llvm-objdump, and every function symbol's instruction text is digested after two
normalisations that depend on where the function lies in its code object, not on what
it does:
  * the 32-bit literal of the s_add_u32 / s_addc_u32 pair that follows an s_getpc_b64
    (the distance to a constant table or a callee);
  * trailing padding (s_nop / s_code_end after the last instruction).
Prints one line per symbol (instruction count, both digests), lists the symbols present
on one side only, and exits 1 if a symbol present on both sides differs.
"""
import hashlib
import os
import re
import shutil
import struct
import subprocess
import sys
import tempfile

LLVM = os.environ.get("ROCM_LLVM_BIN", "/opt/rocm/lib/llvm/bin")
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
EM_AMDGPU = 224


def code_objects(path):
    """The gfx950 code objects (bytes) in `path`."""
    data = open(path, "rb").read()
    if data[:4] == b"\x7fELF" and struct.unpack_from("<H", data, 18)[0] == EM_AMDGPU:
        return [data]
    if data[:4] == b"\x7fELF":  # a host object or library: the bundles are in .hip_fatbin
        with tempfile.TemporaryDirectory() as t:
            fat = os.path.join(t, "fat.bin")
            subprocess.check_call([os.path.join(LLVM, "llvm-objcopy"), "--dump-section=.hip_fatbin=" + fat, path,
                                   os.path.join(t, "x.o")])
            data = open(fat, "rb").read()
    out = []
    at = data.find(MAGIC)
    if at < 0:
        sys.exit("%s: no offload bundle (a compressed bundle is not supported)" % path)
    while at >= 0:
        (n,) = struct.unpack_from("<Q", data, at + len(MAGIC))
        p = at + len(MAGIC) + 8
        for _ in range(n):
            off, size, idlen = struct.unpack_from("<QQQ", data, p)
            ident = data[p + 24:p + 24 + idlen].decode()
            p += 24 + idlen
            if "gfx950" in ident and size:
                out.append(data[at + off:at + off + size])
        at = data.find(MAGIC, p)
    return out


INSN = re.compile(r"^\s+([a-z_0-9]+)(\s.*)?$")
LABEL = re.compile(r"^(?:[0-9a-f]+ )?<([^>]+)>:$")
LITERAL = re.compile(r",\s*(0x[0-9a-f]+|-?[0-9]+)\s*$")
PADDING = ("s_nop", "s_code_end")


def functions(co):
    """{symbol: (is_kernel, [normalised instruction lines])} of one code object."""
    with tempfile.NamedTemporaryFile(suffix=".co") as f:
        f.write(co)
        f.flush()
        syms = subprocess.check_output([os.path.join(LLVM, "llvm-readelf"), "-sW", f.name], text=True)
        text = subprocess.check_output([os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn",
                                        "--no-leading-addr", f.name], text=True)
    kernels = {ln.split()[-1][:-3] for ln in syms.splitlines() if ln.endswith(".kd")}  # kernel descriptors
    out, cur, pc_window = {}, None, 0
    for ln in text.splitlines():
        ln = ln.split("//")[0].rstrip()
        m = LABEL.match(ln)
        if m:
            cur = out.setdefault(m.group(1), (m.group(1) in kernels, []))[1]
            pc_window = 0
            continue
        m = INSN.match(ln)
        if cur is None or not m:
            continue
        op, ins = m.group(1), " ".join(ln.split())
        if op == "s_getpc_b64":
            pc_window = 8
        elif pc_window:
            pc_window -= 1
            if op in ("s_add_u32", "s_addc_u32"):
                ins = LITERAL.sub(", <pc-relative>", ins)
        cur.append(ins)
    for _, body in out.values():
        while body and body[-1].split()[0] in PADDING:
            body.pop()
    return out


def digest_file(path):
    table = {}
    for co in code_objects(path):
        for name, (is_kernel, body) in functions(co).items():
            if name in table:
                sys.exit("%s: symbol %s is defined in two code objects" % (path, name))
            table[name] = (is_kernel, len(body), hashlib.sha256("\n".join(body).encode()).hexdigest()[:16])
    return table


def demangle(names):
    tool = shutil.which("llvm-cxxfilt", path=LLVM) or shutil.which("c++filt")
    if not tool:
        return {n: n for n in names}
    out = subprocess.run([tool], input="\n".join(names), text=True, capture_output=True, check=True).stdout.splitlines()
    return dict(zip(names, out))


def main():
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    a, b = digest_file(sys.argv[1]), digest_file(sys.argv[2])
    nice = demangle(sorted(set(a) | set(b)))
    both = sorted(set(a) & set(b), key=lambda n: nice[n])
    differ = [n for n in both if a[n][2] != b[n][2]]
    print("# a: %s\n# b: %s" % (sys.argv[1], sys.argv[2]))
    print("# kind    insns_a insns_b digest_a         digest_b         same  symbol")
    for n in both:
        print("%-8s %7d %7d  %s %s %-5s %s" % ("kernel" if a[n][0] else "function", a[n][1], b[n][1], a[n][2], b[n][2],
                                               "yes" if a[n][2] == b[n][2] else "NO", nice[n]))
    for side, mine, other in (("a", a, b), ("b", b, a)):
        for n in sorted(set(mine) - set(other), key=lambda n: nice[n]):
            print("only in %s: %-8s %7d  %s  %s" % (side, "kernel" if mine[n][0] else "function", mine[n][1], mine[n][2], nice[n]))
    nk = lambda t: sum(1 for v in t.values() if v[0])
    print("# kernels: a %d, b %d; symbols on both sides %d, equal %d, different %d, only in a %d, only in b %d" %
          (nk(a), nk(b), len(both), len(both) - len(differ), len(differ), len(set(a) - set(b)), len(set(b) - set(a))))
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
