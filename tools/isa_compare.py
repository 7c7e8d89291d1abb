"""Compare the device code of two builds kernel instance by kernel instance.

Both directories hold `hipcc ... --cuda-device-only -S` output, one .s per source file (same flags as windgnn_amd/build.py).
Instances are matched by kernel name and template arguments (an empty trailing argument pack and pgemm_tn_kernel's
PW = false count as absent); lines naming symbols and basic-block numbers are ignored.  Prints MISSING / DIFF per instance
of the first directory and a summary; exit status 1 if any differs.

    python tools/isa_compare.py OLD_DIR NEW_DIR
"""
import re, sys, os
def key(m):
    # _ZN12_GLOBAL__N_1 <len><ident> [I <args> E] E ...   (or _Z<len><ident>...)
    mm = re.match(r'_ZN12_GLOBAL__N_1(\d+)', m) or re.match(r'_Z(\d+)', m)
    if not mm: return m
    n = int(mm.group(1)); i = mm.end(); ident = m[i:i+n]; i += n
    args = []
    if i < len(m) and m[i] == 'I':
        i += 1
        while m[i] != 'E':
            a = re.match(r'L[ib](\d+)E', m[i:])
            if a: args.append(a.group(1)); i += a.end(); continue
            if m[i] == 'J':
                j = m.index('E', i); pack = m[i+1:j]; i = j + 1
                if pack: args.append('pack:' + pack)
                continue
            raise ValueError(m[i:])
    # trailing template defaults that are false: PW = false on pgemm_tn_kernel (5th arg)
    if ident == 'pgemm_tn_kernel' and len(args) == 5 and args[4] == '0': args = args[:4]
    return ident + '<' + ','.join(args) + '>'
def funcs(path):
    out = {}; cur = None; body = []
    for line in open(path):
        m = re.match(r'^(_Z[_A-Za-z0-9]+):', line)
        if m and cur is None and 'kernel' in m.group(1):
            cur = m.group(1); body = []; continue
        if cur is not None:
            if line.startswith('.Lfunc_end'):
                out[key(cur)] = body; cur = None; continue
            s = re.sub(r'\.LBB\d+_', '.LBB_', line.split(';')[0].rstrip())
            if s.strip() and '_Z' not in s: body.append(s)
    return out
if __name__ == '__main__':
    a_dir, b_dir = sys.argv[1], sys.argv[2]
    bad = 0; n = 0
    for f in sorted(os.listdir(a_dir)):
        A = funcs(os.path.join(a_dir, f)); B = funcs(os.path.join(b_dir, f))
        for k, v in A.items():
            n += 1
            if k not in B: print("MISSING", f, k); bad += 1
            elif B[k] != v: print("DIFF", f, k); bad += 1
        new = [k for k in B if k not in A]
        print(f, len(A), "kernel instances at HEAD,", len(new), "new")
    print(n, "instances compared,", bad, "differ")
    sys.exit(1 if bad else 0)
