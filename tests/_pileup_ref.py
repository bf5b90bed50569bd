"""The pileup contract (include/radian_hip.h rd_pileup_*) restated in plain Python, for the tests: per-site channels,
the error profile and the per-pair fields of a batch of pairs, and the files of python -m radian_amd.pileup.  The ops of an aligned pair
come from tests/_align_ref.py's traceback (the fixed tie-break), never from the library."""
import numpy as np

import _align_ref as ar

CHANNELS = ("A", "C", "G", "T", "other", "del", "ins", "starts")
CONF, INS_BASE, KMER, INS_LEN, DEL_LEN, PROFILE_LEN = 0, 30, 35, 35 + 4096, 35 + 4096 + 64, 35 + 4096 + 128
OK, NO_BASE, TOO_LARGE = 0, 1, 2
FIELDS = ("status", "score", "ref_lo", "ref_hi", "clip_head", "clip_tail", "n_match", "n_sub", "n_ins", "n_del")
BASES = "ACGT"


def code(byte):
    return BASES.index(chr(byte)) if chr(byte) in BASES else 4


def kmer(span, i):
    """index of span[i-2 .. i+2], None within 2 of an end or with a non-ACGT byte"""
    if i < 2 or i + 2 >= len(span):
        return None
    cs = [code(b) for b in span[i - 2: i + 3]]
    if max(cs) > 3:
        return None
    k = 0
    for c in cs:
        k = 4 * k + c
    return k


def bucket(length):
    return min(length, 64) - 1


def runs(ops, lo, hi, kind):
    """(start column, length) of the maximal runs of `kind` among columns lo .. hi"""
    out, k = [], lo
    while k <= hi:
        if ops[k] == kind:
            e = k
            while e + 1 <= hi and ops[e + 1] == kind:
                e += 1
            out.append((k, e - k + 1))
            k = e + 1
        else:
            k += 1
    return out


def pair(ops, span, read, site0, sites, prof, score=0):
    """adds one pair to sites (an array [n_sites, 8]) and prof; returns its ten fields"""
    ops, span, read = bytes(ops), bytes(span), bytes(read)
    assert sum(o != ord("I") for o in ops) == len(span) and sum(o != ord("D") for o in ops) == len(read)
    mx = [k for k, o in enumerate(ops) if o in b"MX"]
    if not mx:
        return [NO_BASE, score, 0, 0, len(read), 0, 0, 0, 0, 0]
    lo, hi = mx[0], mx[-1]
    # span / read offset of every column
    ri, qj, i, j = [], [], 0, 0
    for o in ops:
        ri.append(i)
        qj.append(j)
        i += o != ord("I")
        j += o != ord("D")

    def bump(site, ch):
        sites[site0 + site, ch] += 1

    def ctx(i, e):
        k = kmer(span, i)
        if k is not None:
            prof[KMER + 4 * k + e] += 1

    cnt = dict.fromkeys(b"MXID", 0)
    for k in range(lo, hi + 1):
        o = ops[k]
        cnt[o] += 1
        if o in b"MX":
            bump(ri[k], code(read[qj[k]]))
            prof[CONF + 6 * code(span[ri[k]]) + code(read[qj[k]])] += 1
            ctx(ri[k], 0 if o == ord("M") else 1)
        elif o == ord("D"):
            bump(ri[k], 5)
            prof[CONF + 6 * code(span[ri[k]]) + 5] += 1
            ctx(ri[k], 2)
        else:
            prof[INS_BASE + code(read[qj[k]])] += 1
    for _, length in runs(ops, lo, hi, ord("D")):
        prof[DEL_LEN + bucket(length)] += 1
    for start, length in runs(ops, lo, hi, ord("I")):
        prof[INS_LEN + bucket(length)] += 1
        before = max(k for k in range(lo, start) if ops[k] != ord("I"))
        bump(ri[before], 6)
        ctx(ri[before], 3)
    bump(ri[lo], 7)
    return [OK, score, ri[lo], ri[hi] + 1, qj[lo], len(read) - (qj[hi] + 1), cnt[ord("M")], cnt[ord("X")], cnt[ord("I")], cnt[ord("D")]]


def pileup(ops, spans, reads, site0, n_sites, scores=None):
    """(sites uint32 [n_sites, 8], profile uint64 [PROFILE_LEN], out int32 [n, 10]) of a batch"""
    sites = np.zeros((max(n_sites, 1), 8), dtype=np.int64)
    prof = np.zeros(PROFILE_LEN, dtype=np.int64)
    out = np.zeros((len(ops), 10), dtype=np.int32)
    for p in range(len(ops)):
        out[p] = pair(ops[p], spans[p], reads[p], int(site0[p]), sites, prof, 0 if scores is None else int(scores[p]))
    return sites.astype(np.uint32), prof.astype(np.uint64), out


def aligned(spans, reads):
    """(ops, scores) of the pairs by the CPU aligner's fixed tie-break"""
    score, _, ops = ar.align_cpu(spans, reads)
    return [bytes(o) for o in ops], [int(s) for s in score]


def table(sites, min_depth):
    """(site indices, counts rows) at depth >= min_depth"""
    depth = sites[:, :6].astype(np.int64).sum(axis=1)
    idx = np.nonzero(depth >= min_depth)[0]
    return idx.astype(np.uint32), sites[idx]


# ---------------------------------------------------------------------------------------------- the command line's files
def major_of(row, ref_base):
    """the largest of A C G T del ('-'); on a tie the reference base if it is among the tied, otherwise the first in that order"""
    vals = [int(row[0]), int(row[1]), int(row[2]), int(row[3]), int(row[5])]
    names = "ACGT-"
    top = max(vals)
    tied = [names[c] for c in range(5) if vals[c] == top]
    return (ref_base if ref_base in tied else tied[0]), top


def frac(num, den):
    return "%.4f" % (num / den) if den else "0.0000"


def tsv_rows(names, seqs, sites, all_sites=False):
    """pileup.tsv's lines (header first); seqs as the table saw them (upper case, U = T)"""
    out = ["ref_name\tpos\tref_base\tdepth\tA\tC\tG\tT\tother\tdel\tins\tstarts\tmajor\tmajor_frac\tmismatch_frac"]
    s = 0
    for name, seq in zip(names, seqs):
        for pos, b in enumerate(seq):
            row = sites[s]
            s += 1
            depth = int(row[:6].astype(np.int64).sum())
            if depth == 0 and not all_sites:
                continue
            major, top = major_of(row, b)
            ref_count = int(row[BASES.index(b)]) if b in BASES else 0
            out.append("\t".join([name, str(pos), b, str(depth)] + [str(int(v)) for v in row] + [major, frac(top, depth), frac(depth - ref_count, depth)]))
    return out


def variant_rows(names, seqs, sites, min_depth=10, min_frac=0.5):
    out = ["ref_name\tpos\tref_base\ttype\talt\tdepth\tfrac"]
    s = 0
    for name, seq in zip(names, seqs):
        for pos, b in enumerate(seq):
            row = sites[s]
            s += 1
            depth = int(row[:6].astype(np.int64).sum())
            if depth < min_depth:
                continue
            major, top = major_of(row, b)
            if major != b and top >= min_frac * depth:
                out.append("\t".join([name, str(pos), b, "del" if major == "-" else "sub", major, str(depth), frac(top, depth)]))
            if int(row[6]) >= min_frac * depth:
                out.append("\t".join([name, str(pos), b, "ins", "+", str(depth), frac(int(row[6]), depth)]))
    return out


def profile_rows(prof):
    out = ["table\tkey\tcount"]
    outcome = "ACGTN-"
    for a in range(5):
        for b in range(6):
            out.append(f"conf\t{'ACGTN'[a]}>{outcome[b]}\t{int(prof[CONF + 6 * a + b])}")
    for c in range(5):
        out.append(f"ins_base\t{'ACGTN'[c]}\t{int(prof[INS_BASE + c])}")
    for k in range(1024):
        word = "".join(BASES[(k >> (2 * (4 - d))) & 3] for d in range(5))
        for e, nm in enumerate(("match", "sub", "del", "ins")):
            out.append(f"kmer\t{word} {nm}\t{int(prof[KMER + 4 * k + e])}")
    for tab, at in (("ins_len", INS_LEN), ("del_len", DEL_LEN)):
        for b in range(64):
            out.append(f"{tab}\t{'64+' if b == 63 else b + 1}\t{int(prof[at + b])}")
    return out


def cigar(ops, fields, head_extra=0, tail_extra=0):
    """=/X/I/D of the covered interval, S for both clips (extra: read bases outside the aligned part of the read)"""
    mx = [k for k, o in enumerate(ops) if o in b"MX"]
    lo, hi = mx[0], mx[-1]
    parts = []
    if fields[4] + head_extra:
        parts.append(f"{fields[4] + head_extra}S")
    k = lo
    while k <= hi:
        e = k
        while e + 1 <= hi and ops[e + 1] == ops[k]:
            e += 1
        parts.append(f"{e - k + 1}{ {'M': '=', 'X': 'X', 'I': 'I', 'D': 'D'}[chr(ops[k])] }")
        k = e + 1
    if fields[5] + tail_extra:
        parts.append(f"{fields[5] + tail_extra}S")
    return "".join(parts)


def sam_rows(names, seqs, records):
    """records: (read name, read as written, target index, tstart, qstart, qend, ops, fields) of the piled-up pairs with status OK"""
    out = ["@HD\tVN:1.6\tSO:unknown"] + [f"@SQ\tSN:{n}\tLN:{len(s)}" for n, s in zip(names, seqs)]
    for name, read, t, tstart, qstart, qend, ops, f in records:
        out.append("\t".join([name, "0", names[t], str(tstart + int(f[2]) + 1), "255", cigar(ops, [int(v) for v in f], qstart, len(read) - qend), "*", "0", "0",
                              read, "*", f"NM:i:{int(f[7]) + int(f[8]) + int(f[9])}", f"AS:i:{int(f[1])}"]))
    return out


def cli_files(names, seqs, reads, paf_lines, min_depth=10, min_frac=0.5, all_sites=False):
    """the four files of python -m radian_amd.pileup as texts (tsv, variants, profile, sam), the per-pair fields and the number of reads
    skipped as absent from the PAF; reads [(name, sequence as written)], paf_lines without line ends"""
    first = {}
    for line in paf_lines:
        c = line.split("\t")
        if c[4] == "+" and c[0] not in first:
            first[c[0]] = (int(c[2]), int(c[3]), names.index(c[5]), int(c[7]), int(c[8]))
    offsets = np.concatenate([[0], np.cumsum([len(s) for s in seqs])])
    todo = [(n, s) + first[n] for n, s in reads if n in first]
    spans = [seqs[t][ts:te].encode() for _, _, _, _, t, ts, te in todo]
    parts = [s.upper().replace("U", "T")[qs:qe].encode() for _, s, qs, qe, _, _, _ in todo]
    site0 = [int(offsets[t]) + ts for _, _, _, _, t, ts, _ in todo]
    ops, scores = aligned(spans, parts)
    sites, prof, out = pileup(ops, spans, parts, site0, int(offsets[-1]), scores)
    records = [(n, s, t, ts, qs, qe, ops[k], out[k]) for k, (n, s, qs, qe, t, ts, te) in enumerate(todo) if out[k][0] == OK]
    text = lambda rows: "".join(r + "\n" for r in rows)
    return dict(tsv=text(tsv_rows(names, seqs, sites, all_sites)), variants=text(variant_rows(names, seqs, sites, min_depth, min_frac)),
                profile=text(profile_rows(prof)), sam=text(sam_rows(names, seqs, records)), out=out, skipped=len(reads) - len(todo), sites=sites)
