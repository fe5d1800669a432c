"""dev tool: instruction census of one kernel in a hipcc -S listing (needs no GPU).
usage: python tools/isa_census.py file.s KERNEL_NAME_SUBSTRING            the largest backward-branch loop, by mnemonic
       python tools/isa_census.py file.s KERNEL_NAME_SUBSTRING --phases   every loop that holds a barrier, per barrier-to-barrier
                                                                          phase and instruction class (the wave-specialised
                                                                          decode: group A's and group B's generation loops)
The phase table counts mnemonic prefixes only.  A phase runs from one s_barrier to the next in listing order, the first row from
the loop's label to its first barrier and the last from its last barrier to the loop's branch; the side blocks of a phase (the
once-per-64-steps noise pass, the refill) stand in the listing between the same barriers and are counted with it."""
import collections, re, sys

CLASSES = ("FMA", "VALU", "LDS", "VMEM", "SALU", "s_nop", "wait")


def classify(m):
    if m in ("s_nop",):
        return "s_nop"
    if m.startswith(("s_waitcnt", "s_wait_")):
        return "wait"
    if m.startswith(("v_fma", "v_fmac", "v_mac", "v_pk_fma")):
        return "FMA"
    if m.startswith("ds_"):
        return "LDS"
    if m.startswith(("buffer_", "global_", "flat_", "scratch_")):
        return "VMEM"
    if m.startswith("v_"):
        return "VALU"
    if m.startswith("s_"):
        return "SALU"        # scalar ALU, scalar memory, branches, s_barrier, s_setprio ...
    return "VALU"


def kernel_lines(path, name):
    s = open(path).read().split('\n')
    start = next(i for i, l in enumerate(s) if re.match(r'^_Z\S*' + re.escape(name) + r'\S*:', l))
    end = next(i for i in range(start, len(s)) if s[i].strip().startswith('s_endpgm'))
    return s[start].rstrip(':'), [l.strip() for l in s[start:end]]


def backward_branches(lines):
    labels = {re.match(r'^(\.LBB\d+_\d+):', l).group(1): i for i, l in enumerate(lines) if re.match(r'^\.LBB\d+_\d+:', l)}
    back = []
    for i, l in enumerate(lines):
        mm = re.match(r's_c?branch\w*\s+(\.LBB\d+_\d+)', l)
        if mm and mm.group(1) in labels and labels[mm.group(1)] < i:
            back.append((labels[mm.group(1)], i))
    return back


def is_instr(l):
    return bool(l) and not l.startswith(('.', ';')) and not l.endswith(':')


def phases(lines, a, b):
    """[(name, Counter by class)] of the loop lines[a .. b] (b: its backward branch, counted)"""
    rows, cur = [], collections.Counter()
    for l in lines[a:b + 1]:
        if not is_instr(l):
            continue
        m = l.split()[0]
        cur[classify(m)] += 1
        if m == "s_barrier":
            rows.append(cur)
            cur = collections.Counter()
    rows.append(cur)
    return rows


def main():
    name, lines = kernel_lines(sys.argv[1], sys.argv[2])
    back = backward_branches(lines)
    if "--phases" not in sys.argv[3:]:
        print("backward branches (label line, branch line):", back, "kernel lines:", len(lines))
        a, b = max(back, key=lambda x: x[1] - x[0])
        c = collections.Counter(l.split()[0] for l in lines[a:b] if is_instr(l))
        print("loop instructions:", sum(c.values()))
        for k, v in c.most_common(60):
            print(f"{v:5d} {k}")
        return
    print(f"kernel {name}")
    # outermost loops that hold a barrier, in listing order (the two groups are separate bodies, each with a prologue and a
    # generation loop; group B's are the ones with vector-memory loads in the layer phases)
    loops = [(a, b) for a, b in back if any(l.startswith("s_barrier") for l in lines[a:b])]
    loops = [x for x in loops if not any(y != x and y[0] <= x[0] and x[1] <= y[1] for y in loops)]
    for n, (a, b) in enumerate(sorted(loops)):
        rows = phases(lines, a, b)
        total = sum(sum(r.values()) for r in rows)
        print(f"loop {n}: listing lines {a} .. {b}, {len(rows) - 1} barriers, {total} instructions")
        print("  phase              all " + " ".join(f"{c:>6}" for c in CLASSES))
        for k, r in enumerate(rows):
            nm = "head -> barrier 0" if k == 0 else (f"barrier {k - 1} -> branch" if k == len(rows) - 1 else f"barrier {k - 1} -> {k}")
            print(f"  {nm:<18}{sum(r.values()):>4} " + " ".join(f"{r[c]:>6}" for c in CLASSES))


if __name__ == "__main__":
    main()
