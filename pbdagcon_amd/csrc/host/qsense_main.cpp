// qsense -- the q-sense.py command line (src/q-sense.py) on the device: consensus of a cluster of reads of one template.
//
// q-sense.py picks a seed (d: by self-to-self alignment, r: the first record of a reference FASTA), then repeats align ->
// DAG consensus --n_iter times (q-sense.py:36-72, 78-127); its pbtools.pbdagcon.q_sense module and blasr are not in the
// reference tree, so everything below is this build's own: PARITY UNPINNED.  Per round, for every cluster at once:
//   seed       d: dagcon_place on every ordered pair of the first --max_n_reads reads; the read with the largest sum of
//              max(V+, V-) over the reads placed on it (the smaller index on a tie).  Written to {prefix}_ref.fa
//   place      every read on the seed (dagcon_place); reads unplaced or with max(V) < 3 are dropped, at most --max_cov
//              kept, by support descending, then index
//   align      '-' reads reverse-complemented, aligned with local ends (dagcon_align, DAGCON_FLAG_LOCAL_ALIGN) to the seed
//              window [t0 - 96, t1 + 96); start = window start + t_begin + 1
//   consensus  dagcon_consensus with the seed as the real backbone (dazcon.cpp:76), min_cov = min_weight = --min_cov,
//              trim 10; the longest segment (the first on a tie) is the next round's seed
// A cluster stops early when its consensus comes back unchanged.
#include <algorithm>
#include <cerrno>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "../../../include/dagcon.h"

namespace {

const uint32_t K = 12, MAX_OCC = 4, MIN_VOTES = 3, FLANK = 96, TRIM = 10;

struct Opts {
    char mode = 0;
    std::string input, ref, fofn, out = "g_consensus", dir = "./", cname = "consensus";
    uint32_t n_iter = 4, min_cov = 8, max_cov = 60, max_n_reads = 150, min_len = 100;
    int device = 0;
};

void usage(FILE *f) {
    fprintf(f,
            "usage: qsense {d,r} [options] input.fasta [ref.fasta]\n"
            "       qsense {d,r} [options] --fofn FILE\n"
            "\n"
            "Consensus of a cluster of reads of one template, on the GPU: the q-sense.py command line.  q-sense.py's\n"
            "aligner (blasr) and its pbtools module are not in the reference tree: parity unpinned.  This code is\n"
            "designed for consensus up to the length of reads; it is not optimized for larger templates (every read\n"
            "and seed at most 65,536 bases).\n"
            "\n"
            "  d input.fasta            seed picked by self-to-self placement of the reads\n"
            "  r input.fasta ref.fasta  seed: the first record of ref.fasta\n"
            "\n"
            "  -o, --output NAME        consensus output file name (g_consensus): {dir}/{NAME without its last .ext}.fa\n"
            "  -d, --output_dir DIR     output directory (./)\n"
            "  --cname NAME             consensus sequence name (consensus)\n"
            "  --n_iter N               rounds of consensus correction (4)\n"
            "  --min_cov N              minimum coverage for a consensus (8)\n"
            "  --max_cov N              maximum reads used for a consensus (60)\n"
            "  --max_n_reads N          reads of a cluster considered (150)\n"
            "  --nproc N                accepted and ignored\n"
            "  --min_len N              shortest alignment and consensus segment used (100; this build's addition)\n"
            "  --fofn FILE              one cluster a line, all clusters batched on the device (this build's addition):\n"
            "                           'input.fasta' for d, 'input.fasta ref.fasta' for r; records are {cname}/{line}\n"
            "  --device N               HIP device (0)\n"
            "  -h, --help               this text\n"
            "\n"
            "Not built: --enable_hp_correction, --hp_correction_th, --mark_lower_case, --dump_dag_info (their behaviour\n"
            "lives in the pbtools package).\n"
            "\n"
            "Exit status: 0 (a cluster that gets no consensus is a warning on stderr), 1 on an I/O, device or write\n"
            "error, 2 on a usage error or an option that is not built.\n");
}

bool parse_uint(const std::string &s, uint32_t *out) {
    if (s.empty()) return false;
    char *e = nullptr;
    errno = 0;
    const unsigned long long v = strtoull(s.c_str(), &e, 10);
    if (*e || errno || v > 0xFFFFFFFFull || s[0] == '-') return false;
    *out = (uint32_t)v;
    return true;
}

// 0: parsed, else the exit status
int parse(int argc, char **argv, Opts &o) {
    if (argc < 2) { usage(stderr); return 2; }
    const std::string m = argv[1];
    if (m == "-h" || m == "--help") { usage(stdout); exit(0); }
    if (m != "d" && m != "r") { fprintf(stderr, "qsense: the first argument is d or r, not '%s'\n", m.c_str()); usage(stderr); return 2; }
    o.mode = m[0];
    std::vector<std::string> pos;
    for (int i = 2; i < argc; i++) {
        std::string a = argv[i], val;
        bool has_val = false;
        if (a.size() > 2 && a[0] == '-' && a[1] == '-' && a.find('=') != std::string::npos) {
            val = a.substr(a.find('=') + 1); a = a.substr(0, a.find('=')); has_val = true;
        }
        auto need = [&](std::string *dst) -> bool {
            if (has_val) { *dst = val; return true; }
            if (i + 1 >= argc) { fprintf(stderr, "qsense: %s needs a value\n", a.c_str()); return false; }
            *dst = argv[++i];
            return true;
        };
        auto need_u = [&](uint32_t *dst) -> bool {
            std::string v;
            if (!need(&v)) return false;
            if (!parse_uint(v, dst)) { fprintf(stderr, "qsense: %s needs an unsigned integer, not '%s'\n", a.c_str(), v.c_str()); return false; }
            return true;
        };
        uint32_t u = 0;
        std::string ignored;
        if (a == "-h" || a == "--help") { usage(stdout); exit(0); }
        else if (a == "--enable_hp_correction" || a == "--hp_correction_th" || a == "--mark_lower_case" || a == "--dump_dag_info") {
            fprintf(stderr, "qsense: %s is not built: homopolymer correction, lower-case marking and DAG dumps live in the "
                            "pbtools package, which this build does not have\n", a.c_str());
            return 2;
        }
        else if (a == "-o" || a == "--output") { if (!need(&o.out)) return 2; }
        else if (a == "-d" || a == "--output_dir") { if (!need(&o.dir)) return 2; }
        else if (a == "--cname") { if (!need(&o.cname)) return 2; }
        else if (a == "--n_iter") { if (!need_u(&o.n_iter)) return 2; }
        else if (a == "--min_cov") { if (!need_u(&o.min_cov)) return 2; }
        else if (a == "--max_cov") { if (!need_u(&o.max_cov)) return 2; }
        else if (a == "--max_n_reads") { if (!need_u(&o.max_n_reads)) return 2; }
        else if (a == "--min_len") { if (!need_u(&o.min_len)) return 2; }
        else if (a == "--nproc") { if (!need(&ignored)) return 2; }
        else if (a == "--fofn") { if (!need(&o.fofn)) return 2; }
        else if (a == "--device") { if (!need_u(&u)) return 2; o.device = (int)u; }
        else if (a.size() > 1 && a[0] == '-') { fprintf(stderr, "qsense: unknown argument %s\n", a.c_str()); usage(stderr); return 2; }
        else pos.push_back(a);
    }
    const size_t want = (o.fofn.empty() ? 1 : 0) + (o.mode == 'r' && o.fofn.empty() ? 1 : 0);
    if (pos.size() != want) {
        fprintf(stderr, "qsense: %s expects %s\n", o.mode == 'd' ? "d" : "r",
                !o.fofn.empty() ? "no input file with --fofn" : o.mode == 'd' ? "input.fasta" : "input.fasta ref.fasta");
        usage(stderr);
        return 2;
    }
    if (o.fofn.empty()) { o.input = pos[0]; if (o.mode == 'r') o.ref = pos[1]; }
    if (o.n_iter == 0) o.n_iter = 1;
    return 0;
}

struct Rec { std::string name, seq; };

bool read_fasta(const std::string &path, std::vector<Rec> &out, std::string &err) {
    std::ifstream in(path, std::ios::binary);
    if (!in) { err = "cannot open " + path; return false; }
    std::string line;
    while (std::getline(in, line)) {
        if (!line.empty() && line.back() == '\r') line.pop_back();
        if (line.empty()) continue;
        if (line[0] == '>') { out.push_back(Rec{line.substr(1), std::string()}); continue; }
        if (out.empty()) { err = path + " is not FASTA (sequence before the first '>')"; return false; }
        for (char ch : line) if (ch != ' ' && ch != '\t') out.back().seq.push_back(ch);
    }
    if (in.bad()) { err = "error reading " + path; return false; }
    return true;
}

std::string revcomp(const std::string &s) {
    std::string r(s.rbegin(), s.rend());
    for (char &ch : r) {
        switch (ch) {
            case 'A': ch = 'T'; break; case 'C': ch = 'G'; break; case 'G': ch = 'C'; break; case 'T': ch = 'A'; break;
            case 'a': ch = 't'; break; case 'c': ch = 'g'; break; case 'g': ch = 'c'; break; case 't': ch = 'a'; break;
            default: break;
        }
    }
    return r;
}

// q-sense.py:79-86: the output name without its last extension, joined to the directory as os.path.join does
std::string full_prefix(const Opts &o) {
    std::string p = o.out;
    const size_t dot = p.rfind('.');
    if (dot != std::string::npos) p = p.substr(0, dot);
    if (!p.empty() && p[0] == '/') return p;
    if (o.dir.empty()) return p;
    return o.dir.back() == '/' ? o.dir + p : o.dir + "/" + p;
}

struct Cluster {
    std::vector<std::string> reads;   // the first --max_n_reads
    std::string seed, cns;
    bool active = true, have_cns = false;
};

// every (query, target) pair through dagcon_place, over the sequences seqs
struct Placement { std::vector<uint32_t> vf, vr, t0, t1; std::vector<char> strand; };
int place(dagcon_ctx *ctx, const std::vector<const std::string *> &seqs, const std::vector<uint32_t> &pq,
          const std::vector<uint32_t> &pt, Placement &pl) {
    std::vector<uint64_t> off;
    std::vector<uint32_t> len;
    std::string blob;
    for (const std::string *s : seqs) { off.push_back(blob.size()); len.push_back((uint32_t)s->size()); blob += *s; }
    const size_t n = pq.size();
    pl.vf.assign(n, 0); pl.vr.assign(n, 0); pl.t0.assign(n, 0); pl.t1.assign(n, 0); pl.strand.assign(n, '.');
    if (!n) return DAGCON_OK;
    return dagcon_place(ctx, off.data(), len.data(), blob.data(), blob.size(), (uint32_t)n, pq.data(), pt.data(), K, MAX_OCC,
                        pl.vf.data(), pl.vr.data(), pl.strand.data(), pl.t0.data(), pl.t1.data());
}

bool fits(const std::string &s) { return s.size() <= DAGCON_PLACE_MAX_LEN; }

}  // namespace

int main(int argc, char **argv) {
    Opts o;
    if (int rc = parse(argc, argv, o)) return rc;

    // ---- inputs ----
    std::vector<std::pair<std::string, std::string>> jobs;      // (reads, ref)
    if (o.fofn.empty()) {
        jobs.push_back({o.input, o.ref});
    } else {
        std::ifstream in(o.fofn);
        if (!in) { fprintf(stderr, "qsense: cannot open %s\n", o.fofn.c_str()); return 1; }
        std::string line;
        while (std::getline(in, line)) {
            std::istringstream ss(line);
            std::string a, b, extra;
            if (!(ss >> a)) continue;
            ss >> b;
            if ((o.mode == 'r') != !b.empty() || (ss >> extra)) {
                fprintf(stderr, "qsense: %s: a line holds %s\n", o.fofn.c_str(), o.mode == 'r' ? "input.fasta ref.fasta" : "input.fasta");
                return 1;
            }
            jobs.push_back({a, b});
        }
    }
    const bool named = !o.fofn.empty();
    auto cname_of = [&](size_t g, const char *suffix) {
        return o.cname + suffix + (named ? "/" + std::to_string(g) : std::string());
    };
    std::vector<Cluster> cl(jobs.size());
    for (size_t g = 0; g < jobs.size(); g++) {
        std::vector<Rec> recs;
        std::string err;
        if (!read_fasta(jobs[g].first, recs, err)) { fprintf(stderr, "qsense: %s\n", err.c_str()); return 1; }
        for (size_t i = 0; i < recs.size() && i < o.max_n_reads; i++) cl[g].reads.push_back(std::move(recs[i].seq));
        if (o.mode == 'r') {
            std::vector<Rec> ref;
            if (!read_fasta(jobs[g].second, ref, err)) { fprintf(stderr, "qsense: %s\n", err.c_str()); return 1; }
            if (ref.empty()) { fprintf(stderr, "qsense: %s holds no record\n", jobs[g].second.c_str()); return 1; }
            cl[g].seed = ref[0].seq;
        }
        bool ok = !cl[g].reads.empty() && fits(cl[g].seed);
        for (const std::string &r : cl[g].reads) ok &= fits(r);
        if (!ok) {
            fprintf(stderr, "qsense: warning: cluster %zu (%s): %s; no consensus\n", g, jobs[g].first.c_str(),
                    cl[g].reads.empty() ? "no reads" : "a read or the seed is longer than 65,536 bases");
            cl[g].active = false;
        }
    }

    dagcon_ctx *ctx = nullptr;
    dagcon_opts dopt;
    dagcon_default_opts(&dopt);
    dopt.min_cov = o.min_cov; dopt.min_len = o.min_len; dopt.trim = TRIM; dopt.min_weight = (int32_t)o.min_cov;
    dopt.device = o.device; dopt.flags = DAGCON_FLAG_LOCAL_ALIGN;
    if (int rc = dagcon_create(&dopt, &ctx)) {
        fprintf(stderr, "qsense: no usable MI355X as device %d (dagcon_create = %d); there is no CPU fallback\n", o.device, rc);
        return 1;
    }
    auto device_error = [&](const char *what, int rc) {
        fprintf(stderr, "qsense: %s failed (%d): %s\n", what, rc, dagcon_last_error(ctx));
        dagcon_destroy(ctx);
        return 1;
    };
    const std::string prefix = full_prefix(o);

    // ---- d: the seed by all-against-all placement ----
    if (o.mode == 'd') {
        std::vector<const std::string *> seqs;
        std::vector<uint32_t> pq, pt, base(cl.size(), 0);
        for (size_t g = 0; g < cl.size(); g++) {
            if (!cl[g].active) continue;
            base[g] = (uint32_t)seqs.size();
            const uint32_t n = (uint32_t)cl[g].reads.size();
            for (const std::string &r : cl[g].reads) seqs.push_back(&r);
            for (uint32_t i = 0; i < n; i++)
                for (uint32_t j = 0; j < n; j++)
                    if (j != i) { pq.push_back(base[g] + j); pt.push_back(base[g] + i); }
        }
        Placement pl;
        if (int rc = place(ctx, seqs, pq, pt, pl)) return device_error("dagcon_place", rc);
        std::vector<uint64_t> score(seqs.size(), 0);
        for (size_t a = 0; a < pq.size(); a++) score[pt[a]] += std::max(pl.vf[a], pl.vr[a]);
        FILE *f = fopen((prefix + "_ref.fa").c_str(), "w");
        if (!f) { fprintf(stderr, "qsense: cannot write %s_ref.fa\n", prefix.c_str()); dagcon_destroy(ctx); return 1; }
        for (size_t g = 0; g < cl.size(); g++) {
            if (!cl[g].active) continue;
            uint32_t best = 0;
            for (uint32_t i = 1; i < cl[g].reads.size(); i++) if (score[base[g] + i] > score[base[g] + best]) best = i;
            cl[g].seed = cl[g].reads[best];
            fprintf(f, ">%s\n%s\n", cname_of(g, "_ref").c_str(), cl[g].seed.c_str());
        }
        const bool bad = fflush(f) != 0 || ferror(f);
        if (fclose(f) != 0 || bad) { fprintf(stderr, "qsense: error writing %s_ref.fa\n", prefix.c_str()); dagcon_destroy(ctx); return 1; }
    }

    // ---- the rounds ----
    for (uint32_t round = 0; round < o.n_iter; round++) {
        std::vector<size_t> act;
        for (size_t g = 0; g < cl.size(); g++) if (cl[g].active) act.push_back(g);
        if (act.empty()) break;
        auto drop = [&](size_t g, const char *why) {
            fprintf(stderr, "qsense: warning: cluster %zu (%s), round %u: %s; %s\n", g, jobs[g].first.c_str(), round + 1, why,
                    cl[g].have_cns ? "keeping the last round's consensus" : "no consensus");
            cl[g].active = false;
        };
        // place every read on the seed
        std::vector<const std::string *> seqs;
        std::vector<uint32_t> pq, pt, first(act.size() + 1, 0);
        for (size_t x = 0; x < act.size(); x++) {
            Cluster &c = cl[act[x]];
            const uint32_t s = (uint32_t)seqs.size();
            seqs.push_back(&c.seed);
            first[x] = (uint32_t)pq.size();
            for (const std::string &r : c.reads) { pq.push_back((uint32_t)seqs.size()); pt.push_back(s); seqs.push_back(&r); }
        }
        first[act.size()] = (uint32_t)pq.size();
        Placement pl;
        if (int rc = place(ctx, seqs, pq, pt, pl)) return device_error("dagcon_place", rc);
        // select, cut the windows, align
        struct Job { size_t x; uint32_t w0; };
        std::vector<Job> aj;
        std::string qb, tb;
        std::vector<uint64_t> qo, to, oo;
        std::vector<uint32_t> ql, tl;
        uint64_t room = 0;
        for (size_t x = 0; x < act.size(); x++) {
            Cluster &c = cl[act[x]];
            std::vector<uint32_t> keep;
            for (uint32_t a = first[x]; a < first[x + 1]; a++)
                if (pl.strand[a] != '.' && std::max(pl.vf[a], pl.vr[a]) >= MIN_VOTES) keep.push_back(a);
            std::stable_sort(keep.begin(), keep.end(), [&](uint32_t a, uint32_t b) {
                return std::max(pl.vf[a], pl.vr[a]) > std::max(pl.vf[b], pl.vr[b]);
            });
            if (keep.size() > o.max_cov) keep.resize(o.max_cov);
            if (keep.size() < o.min_cov) { drop(act[x], "fewer than --min_cov reads placed on the seed"); continue; }
            for (uint32_t a : keep) {
                const std::string &r = c.reads[a - first[x]];
                const std::string q = pl.strand[a] == '-' ? revcomp(r) : r;
                const uint32_t w0 = pl.t0[a] > FLANK ? pl.t0[a] - FLANK : 0;
                const uint32_t w1 = (uint32_t)std::min<uint64_t>(c.seed.size(), (uint64_t)pl.t1[a] + FLANK);
                if (w1 <= w0) continue;
                aj.push_back(Job{x, w0});
                qo.push_back(qb.size()); ql.push_back((uint32_t)q.size()); qb += q;
                to.push_back(tb.size()); tl.push_back(w1 - w0); tb.append(c.seed, w0, w1 - w0);
                oo.push_back(room); room += (uint64_t)ql.back() + tl.back();
            }
        }
        const uint32_t na = (uint32_t)aj.size();
        std::vector<char> qa(room + 1), ta(room + 1);
        std::vector<uint32_t> alen(na + 1), qbeg(na + 1), qend(na + 1), tbeg(na + 1), tend(na + 1);
        if (na) {
            if (int rc = dagcon_align(ctx, na, qo.data(), ql.data(), to.data(), tl.data(), qb.data(), qb.size(), tb.data(), tb.size(),
                                      oo.data(), qa.data(), ta.data(), alen.data()))
                return device_error("dagcon_align", rc);
            if (int rc = dagcon_align_ends(ctx, na, qbeg.data(), qend.data(), tbeg.data(), tend.data()))
                return device_error("dagcon_align_ends", rc);
        }
        // the consensus batch: one target per cluster that still has --min_cov alignments
        std::vector<std::vector<uint32_t>> per(act.size());
        for (uint32_t a = 0; a < na; a++) if (alen[a]) per[aj[a].x].push_back(a);
        std::vector<size_t> tx;
        for (size_t x = 0; x < act.size(); x++) {
            if (!cl[act[x]].active) continue;
            if (per[x].size() < o.min_cov) { drop(act[x], "fewer than --min_cov reads aligned to the seed"); continue; }
            tx.push_back(x);
        }
        if (tx.empty()) continue;
        std::vector<uint32_t> tlen, start, len;
        std::vector<uint64_t> begin{0}, off, bb_off;
        std::string q, t, bb;
        for (size_t x : tx) {
            const Cluster &c = cl[act[x]];
            tlen.push_back((uint32_t)c.seed.size());
            bb_off.push_back(bb.size());
            bb += c.seed;
            for (uint32_t a : per[x]) {
                start.push_back(aj[a].w0 + tbeg[a] + 1);
                off.push_back(q.size()); len.push_back(alen[a]);
                q.append(qa.data() + oo[a], alen[a]); t.append(ta.data() + oo[a], alen[a]);
            }
            begin.push_back(start.size());
        }
        dagcon_batch db;
        memset(&db, 0, sizeof db);
        db.n_targets = (uint32_t)tx.size();
        db.tlen = tlen.data(); db.aln_begin = begin.data(); db.aln_start = start.data();
        db.aln_off = off.data(); db.aln_len = len.data(); db.qstr = q.data(); db.tstr = t.data(); db.blob_bytes = q.size();
        db.backbone = bb.data(); db.backbone_off = bb_off.data();
        dagcon_results r;
        if (int rc = dagcon_consensus(ctx, &db, &r)) return device_error("dagcon_consensus", rc);
        for (uint32_t y = 0; y < r.n_targets; y++) {
            Cluster &c = cl[act[tx[y]]];
            if (r.target_status[y] != DAGCON_OK) { drop(act[tx[y]], "the consensus failed on the device"); continue; }
            uint64_t best = r.seg_begin[y];
            for (uint64_t s = r.seg_begin[y]; s < r.seg_begin[y + 1]; s++) if (r.seq_len[s] > r.seq_len[best]) best = s;
            if (best == r.seg_begin[y + 1]) { drop(act[tx[y]], "no consensus segment"); continue; }
            std::string cns(r.seq_blob + r.seq_off[best], r.seq_len[best]);
            if (!fits(cns)) { c.cns = cns; c.have_cns = true; drop(act[tx[y]], "the consensus is longer than 65,536 bases"); continue; }
            if (cns == c.seed) c.active = false;                            // converged
            c.seed = c.cns = cns;
            c.have_cns = true;
        }
    }
    dagcon_destroy(ctx);

    // ---- {prefix}.fa ----
    const std::string path = prefix + ".fa";
    FILE *f = fopen(path.c_str(), "w");
    if (!f) { fprintf(stderr, "qsense: cannot write %s\n", path.c_str()); return 1; }
    for (size_t g = 0; g < cl.size(); g++)
        if (cl[g].have_cns) fprintf(f, ">%s\n%s\n", cname_of(g, "").c_str(), cl[g].cns.c_str());
    const bool bad = fflush(f) != 0 || ferror(f);
    if (fclose(f) != 0 || bad) { fprintf(stderr, "qsense: error writing %s\n", path.c_str()); return 1; }
    return 0;
}
