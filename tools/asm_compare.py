"""Developer tool: compares two gfx950 assembly files (hipcc --cuda-device-only -S) kernel by kernel.

    python tools/asm_compare.py parent.s new.s

Per kernel: instruction count, VGPRs, SGPRs, LDS, scratch and occupancy of both files, and whether the instruction streams
are identical after stripping labels, comments and directives; for kernels that differ, the opcodes whose counts changed."""
import collections
import re
import subprocess
import sys


def demangle(name):
    try:
        return subprocess.run(["c++filt", name], capture_output=True, text=True).stdout.strip() or name
    except OSError:
        return name


def kernels(path):
    out, name, body = {}, None, []
    for line in open(path):
        m = re.match(r"^([A-Za-z_][\w$.]*):", line)
        if m and not m.group(1).startswith(".L"):
            name, body = m.group(1), []
            out[name] = dict(body=body)
            continue
        c = re.match(r"^;\s*(NumVgprs|TotalNumSgprs|ScratchSize|Occupancy|LDSByteSize):\s*(\d+)", line.strip())
        if c and name:
            out[name].setdefault(c.group(1), int(c.group(2)))
        s = line.split(";")[0].strip()                     # (a comment line leaves nothing)
        if name is None or not s or s.startswith(".") or re.match(r"^[.\w$]+:$", s):
            continue
        # branch targets are labels numbered per file: keep the opcode only
        s = re.sub(r"\.LBB\d+_\d+", "L", s)
        body.append(s)
    # keyed by the kernel's name without its parameter list: a parameter type that moved to another namespace is the same kernel
    return {demangle(k).replace("(anonymous namespace)::", "").split("(")[0]: v for k, v in out.items() if "NumVgprs" in v}


def main():
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    same = 0
    for k in a:
        if k not in b:
            print(f"{k}: only in {sys.argv[1]}")
            continue
        ka, kb = a[k], b[k]
        ident = ka["body"] == kb["body"]
        same += ident
        print(f"{k}: {'identical' if ident else 'DIFFERS'}")
        for tag, kk in (("parent", ka), ("new", kb)):
            print(f"    {tag:6s} {len(kk['body']):5d} instructions, {kk['NumVgprs']:3d} VGPRs, {kk['TotalNumSgprs']:3d} SGPRs, "
                  f"LDS {kk.get('LDSByteSize', 0):5d} B, scratch {kk['ScratchSize']}, occupancy {kk['Occupancy']}")
        if not ident:
            ca = collections.Counter(s.split()[0] for s in ka["body"])
            cb = collections.Counter(s.split()[0] for s in kb["body"])
            d = {op: (ca[op], cb[op]) for op in sorted(set(ca) | set(cb)) if ca[op] != cb[op]}
            print("    opcode counts that differ (parent -> new): " + (", ".join(f"{op} {x} -> {y}" for op, (x, y) in d.items()) or
                                                                      "none: the same opcodes in another order / other registers"))
    for k in b:
        if k not in a:
            print(f"{k}: only in {sys.argv[2]}")
    print(f"{len(a)} / {len(b)} kernels, identical {same}")


if __name__ == "__main__":
    main()
