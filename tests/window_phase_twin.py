"""The read labels of neighbouring windows joined into blocks (include/dagcon.h, rule 9), in plain Python with
dictionaries: nothing here assumes an order of the alignments, the sites or the records.  `link` is the rule on the
arrays of dagcon_fetch_site_reads; `record_labels` and `haplotag_line` are pbdagcon --phase-windows' vote per record."""

MIN_LINKS, MAX_CONFLICT_PPM = 3, 250000


def linked(same, diff, min_links=0, max_conflict_ppm=0):
    """Rule 9.3 on a window's two counts (Python integers: no width to overflow)."""
    ml, ppm = min_links or MIN_LINKS, max_conflict_ppm or MAX_CONFLICT_PPM
    hi, lo = max(same, diff), min(same, diff)
    return hi >= ml and hi > lo and lo * 1000000 <= ppm * (hi + lo)


def link(win_target, aln_tgt, aln_src, hap, site_tgt, phase, min_links=0, max_conflict_ppm=0):
    """win_target[w]: the target window w lies on.  aln_tgt / aln_src / hap: per taken alignment its window, its record
    and its label in the window's own names.  site_tgt / phase: per site its window and its phase.  Returns the six
    arrays (lists): same, diff, block, flip per window, the oriented hap per alignment, the oriented phase per site."""
    W = len(win_target)
    by_win = {}
    for w, r, h in zip(aln_tgt, aln_src, hap):
        d = by_win.setdefault(int(w), {})
        assert int(r) not in d, "a record has at most one piece per window"
        d[int(r)] = int(h)
    same, diff, block, flip = [0] * W, [0] * W, list(range(W)), [0] * W
    for w in range(W):
        if w == 0 or win_target[w] != win_target[w - 1]:
            continue
        prev, cur = by_win.get(w - 1, {}), by_win.get(w, {})
        for r, h in cur.items():
            g = prev.get(r, 0)
            if h and g:
                if h == g:
                    same[w] += 1
                else:
                    diff[w] += 1
        if linked(same[w], diff[w], min_links, max_conflict_ppm):
            flip[w] = flip[w - 1] ^ (1 if diff[w] > same[w] else 0)
            block[w] = block[w - 1]
    ohap = [int(h) if not h or not flip[int(w)] else 3 - int(h) for w, h in zip(aln_tgt, hap)]
    ophase = [-int(s) if flip[int(w)] else int(s) for w, s in zip(site_tgt, phase)]
    return same, diff, block, flip, ohap, ophase


def vote(pieces):
    """pieces: [(block, oriented label)] of one record.  (HAP, block) -- block None when no piece is labelled."""
    per = {}
    for b, h in pieces:
        if h:
            n, v = per.get(b, (0, 0))
            per[b] = (n + 1, v + (1 if h == 1 else -1))
    if not per:
        return 0, None
    b = min(per, key=lambda k: (-per[k][0], k))
    v = per[b][1]
    return (1 if v > 0 else 2 if v < 0 else 0), b


def record_labels(aln_tgt, aln_src, ohap, block):
    """Per record with a taken piece (a dict by record): (HAP, block or None)."""
    pieces = {}
    for w, r, h in zip(aln_tgt, aln_src, ohap):
        pieces.setdefault(int(r), []).append((int(block[int(w)]), int(h)))
    return {r: vote(p) for r, p in pieces.items()}


def haplotag_line(rname, qname, hap, sites, ps):
    """ps: 1 + the core begin of the block's first window, None without a labelled piece."""
    return "\t".join([rname, qname, str(hap), str(sites), "." if ps is None else str(ps)])
