#!/usr/bin/env python3
"""Static instruction counts of a kernel's largest depth-2 loop in a device listing (rounds 5-7).

  hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -Iinclude --cuda-device-only -S shenqi_amd/csrc/grav_walk.hip -o walk.s
  python tools/listing_counts.py walk.s grav_pair_kernel

For every function whose mangled name contains one of the given words: registers and scratch from the resource comments behind the
function, and the counts over the basic blocks that the compiler's loop comments assign to the depth-2 loop with the most instructions
(for the pair kernel: the round loop of grav_pair_body; rare branches included, a static count, not what a wave executes)."""
import collections
import re
import sys


def functions(lines):
    funcs, res, cur = {}, {}, None
    for ln in lines:
        m = re.match(r"^(_Z\w+):", ln)
        if m:
            cur = m.group(1)
            funcs[cur], res[cur] = [], {}
            continue
        m = re.match(r"^; (NumVgprs|TotalNumSgprs|ScratchSize|Occupancy): (\d+)", ln)
        if m and cur:
            res[cur][m.group(1)] = int(m.group(2))
        if cur and not ln.startswith(";"):
            funcs[cur].append(ln)
    return funcs, res


def blocks(body):
    out, cur = [], dict(label="entry", comment="", ins=[])
    out.append(cur)
    for ln in body:
        m = re.match(r"^(\.LBB\d+_\d+):(.*)", ln)
        if m:
            cur = dict(label=m.group(1)[2:], comment=m.group(2), ins=[])
            out.append(cur)
            continue
        s = ln.strip()
        if s.startswith(";"):
            if not cur["ins"]:
                cur["comment"] += " " + s
            continue
        if s and not s.startswith("."):
            cur["ins"].append(s.split()[0])
    return out


def summary(ins):
    c = collections.Counter(ins)

    def g(pat):
        return sum(n for k, n in c.items() if re.match(pat, k))
    return dict(vector=g(r"v_"), v_mov=g(r"v_mov_b"), v_bcnt=g(r"v_bcnt"), v_mbcnt=g(r"v_mbcnt"), shift64=g(r"v_lshlrev_b64|v_lshl_add_u64"),
                v_cndmask=g(r"v_cndmask"), scalar=g(r"s_(?!waitcnt|nop)"), branches=g(r"s_cbranch|s_branch"), saveexec=g(r"s_\w*saveexec"),
                waitcnt=g(r"s_waitcnt"), vmem=g(r"global_|flat_|buffer_"), scratch=g(r"scratch_"), lds=g(r"ds_"))


def main():
    path, words = sys.argv[1], sys.argv[2:] or ["grav_pair_kernel"]
    funcs, res = functions(open(path).read().split("\n"))
    for name, body in funcs.items():
        if not any(w in name for w in words):
            continue
        bl = blocks(body)
        loops, depth = collections.defaultdict(list), {}
        for b in bl:
            c = b["comment"]
            hs = set(re.findall(r"Header=(BB\d+_\d+)", c)) | set(re.findall(r"Parent Loop (BB\d+_\d+)", c))
            m = re.search(r"Loop Header: Depth=(\d+)", c)
            if m:
                hs.add(b["label"])
                depth[b["label"]] = int(m.group(1))
            for h in hs:
                loops[h] += b["ins"]
        print(name, res.get(name))
        d2 = sorted((len(v), h) for h, v in loops.items() if depth.get(h) == 2)
        if d2:
            print("  largest depth-2 loop (%s): %s" % (d2[-1][1], summary(loops[d2[-1][1]])))


if __name__ == "__main__":
    main()
