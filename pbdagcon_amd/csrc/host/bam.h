// bam.h -- what `pbdagcon --bam --ref` needs of BAM: the BGZF container (a run of gzip members, each with the BC extra
// subfield whose BSIZE gives the member's size), a raw-DEFLATE decoder and CRC32 of this file's own (the project links
// nothing but the HIP runtime), the header's references, and the alignment records one after the other.  Written from
// the SAM/BAM specification (SAMv1, sections 4.1 and 4.2) and RFC 1951 / 1952.
//
// The whole file is inflated into one buffer before the first record is taken: member boundaries are found by hopping
// from header to header, members are inflated on the caller's threads (each into its own stretch of the buffer: ISIZE
// says where), and each member's CRC32 and ISIZE are checked.  Records straddle members freely; in the buffer they lie
// whole.  A record's CIGAR ops and its 4-bit seq field are handed on as they lie (dagcon_upload_cigar_packed takes both
// in BAM's own encoding): no per-base work on the host.
//
// Parity unpinned: no htslib, samtools or pysam was at hand and the reference holds no BAM, so the files in the tests
// come from the suite's own writer (tests/bam_files.py), itself written from the specification.
#pragma once
#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "intake.h"

// ---- CRC32 (RFC 1952, polynomial 0xEDB88320 reflected), a byte at a time ---------------------------------------------
struct DgCrcTable {
    uint32_t t[256];
    DgCrcTable() {
        for (uint32_t i = 0; i < 256; i++) {
            uint32_t c = i;
            for (int k = 0; k < 8; k++) c = (c & 1u) ? 0xEDB88320u ^ (c >> 1) : c >> 1;
            t[i] = c;
        }
    }
};
inline uint32_t dg_crc32(const uint8_t *p, size_t n) {
    static const DgCrcTable tab;
    uint32_t c = 0xFFFFFFFFu;
    for (size_t i = 0; i < n; i++) c = tab.t[(c ^ p[i]) & 0xFFu] ^ (c >> 8);
    return c ^ 0xFFFFFFFFu;
}

// ---- raw DEFLATE (RFC 1951) --------------------------------------------------------------------------------------------
// A code set is held twice: a table indexed by the next DG_INF_ROOT bits of the stream (bit-reversed codes, every code
// of at most that many bits filled in at all its positions: entry = symbol << 4 | length, 0 = no short code here), and
// the canonical counts per length with the symbols in code order, which decode the few longer codes a bit at a time.
#define DG_INF_ROOT 10
struct DgHuff {
    uint16_t fast[1 << DG_INF_ROOT];
    uint16_t count[16];
    uint16_t symbol[288];
    // false: the lengths oversubscribe the code space.  An incomplete set is taken (one distance code of one bit is
    // legal); a code that no symbol has is found when it is met.
    bool build(const uint8_t *len, int n) {
        memset(count, 0, sizeof count);
        memset(fast, 0, sizeof fast);
        for (int s = 0; s < n; s++) count[len[s]]++;
        count[0] = 0;
        int left = 1;
        for (int l = 1; l <= 15; l++) {
            left = (left << 1) - (int)count[l];
            if (left < 0) return false;
        }
        uint16_t offs[16], next[16];
        offs[1] = 0; next[0] = 0;
        uint32_t code = 0;
        for (int l = 1; l <= 15; l++) {
            if (l > 1) offs[l] = (uint16_t)(offs[l - 1] + count[l - 1]);
            code = (code + (l > 1 ? count[l - 1] : 0u)) << 1;
            next[l] = (uint16_t)code;
        }
        for (int s = 0; s < n; s++) {
            const int l = len[s];
            if (!l) continue;
            symbol[offs[l]++] = (uint16_t)s;
            const uint32_t c = next[l]++;
            if (l > DG_INF_ROOT) continue;
            uint32_t r = 0;
            for (int k = 0; k < l; k++) r |= ((c >> k) & 1u) << (l - 1 - k);
            for (uint32_t k = r; k < (1u << DG_INF_ROOT); k += 1u << l) fast[k] = (uint16_t)((s << 4) | l);
        }
        return true;
    }
};

struct DgBits {
    const uint8_t *p, *end;
    uint64_t buf = 0;
    int cnt = 0;
    void fill() { while (cnt <= 56 && p < end) { buf |= (uint64_t)*p++ << cnt; cnt += 8; } }
    // n <= 16 bits, -1 past the end
    int take(int n) {
        if (cnt < n) { fill(); if (cnt < n) return -1; }
        const int v = (int)(buf & ((1u << n) - 1u));
        buf >>= n; cnt -= n;
        return v;
    }
    // the next symbol of h: -1 past the end of the input, -2 a code no symbol has
    int sym(const DgHuff &h) {
        if (cnt < 15) fill();
        const uint16_t e = h.fast[buf & ((1u << DG_INF_ROOT) - 1u)];
        if (e) {
            const int l = e & 15;
            if (l > cnt) return -1;
            buf >>= l; cnt -= l;
            return e >> 4;
        }
        int code = 0, first = 0, index = 0;
        for (int l = 1; l <= 15; l++) {
            if (l > cnt) return -1;
            code |= (int)((buf >> (l - 1)) & 1u);
            const int c = h.count[l];
            if (code - c < first) { buf >>= l; cnt -= l; return h.symbol[index + (code - first)]; }
            index += c; first += c;
            first <<= 1; code <<= 1;
        }
        return -2;
    }
};

struct DgFixedHuff {
    DgHuff lit, dist;
    DgFixedHuff() {
        uint8_t l[288];
        for (int s = 0; s < 288; s++) l[s] = s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : 8;
        lit.build(l, 288);
        for (int s = 0; s < 30; s++) l[s] = 5;
        dist.build(l, 30);
    }
};

// inflates src[0, n) into dst (room for cap bytes); nullptr, or what is wrong with the stream
inline const char *dg_inflate(const uint8_t *src, size_t n, uint8_t *dst, size_t cap, size_t &out_len) {
    static const uint16_t len_base[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
    static const uint8_t len_extra[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
    static const uint16_t dist_base[30] = {1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577};
    static const uint8_t dist_extra[30] = {0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13};
    static const uint8_t cl_order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    static const DgFixedHuff fixed;
    DgBits b;
    b.p = src; b.end = src + n;
    size_t o = 0;
    out_len = 0;
    DgHuff dl, dd;
    for (int last = 0; !last;) {
        last = b.take(1);
        const int type = b.take(2);
        if (last < 0 || type < 0) return "the compressed data ends inside a block header";
        if (type == 3) return "invalid block type";
        if (type == 0) {
            // stored: to the next byte of the input, LEN, its complement, LEN bytes
            b.p -= b.cnt / 8; b.buf = 0; b.cnt = 0;
            if (b.end - b.p < 4) return "the compressed data ends inside a stored block";
            const uint32_t ln = b.p[0] | (uint32_t)b.p[1] << 8, nl = b.p[2] | (uint32_t)b.p[3] << 8;
            b.p += 4;
            if ((ln ^ nl) != 0xFFFFu) return "a stored block's length does not match its complement";
            if ((size_t)(b.end - b.p) < ln) return "the compressed data ends inside a stored block";
            if (ln > cap - o) return "more data than ISIZE says";
            memcpy(dst + o, b.p, ln);
            b.p += ln; o += ln;
            continue;
        }
        const DgHuff *hl = &fixed.lit, *hd = &fixed.dist;
        if (type == 2) {
            const int hlit = b.take(5), hdist = b.take(5), hclen = b.take(4);
            if (hlit < 0 || hdist < 0 || hclen < 0) return "the compressed data ends inside a block header";
            if (hlit + 257 > 286 || hdist + 1 > 30) return "invalid Huffman code (too many length or distance symbols)";
            uint8_t l[320];
            memset(l, 0, 19);
            for (int i = 0; i < hclen + 4; i++) {
                const int v = b.take(3);
                if (v < 0) return "the compressed data ends inside a block header";
                l[cl_order[i]] = (uint8_t)v;
            }
            if (!dl.build(l, 19)) return "invalid Huffman code (code lengths oversubscribed)";
            const DgHuff cl = dl;
            const int total = hlit + 257 + hdist + 1;
            for (int i = 0; i < total;) {
                const int s = b.sym(cl);
                if (s == -1) return "the compressed data ends inside a block header";
                if (s < 0) return "invalid Huffman code";
                if (s < 16) { l[i++] = (uint8_t)s; continue; }
                int rep, v = 0;
                if (s == 16) {
                    if (i == 0) return "invalid Huffman code (a repeat with nothing in front)";
                    v = l[i - 1]; rep = b.take(2); if (rep >= 0) rep += 3;
                } else if (s == 17) { rep = b.take(3); if (rep >= 0) rep += 3; }
                else { rep = b.take(7); if (rep >= 0) rep += 11; }
                if (rep < 0) return "the compressed data ends inside a block header";
                if (i + rep > total) return "invalid Huffman code (a repeat past the last symbol)";
                while (rep--) l[i++] = (uint8_t)v;
            }
            if (l[256] == 0) return "invalid Huffman code (no end-of-block code)";
            if (!dl.build(l, hlit + 257)) return "invalid Huffman code (literal / length codes oversubscribed)";
            if (!dd.build(l + hlit + 257, hdist + 1)) return "invalid Huffman code (distance codes oversubscribed)";
            hl = &dl; hd = &dd;
        }
        for (;;) {
            int s = b.sym(*hl);
            if (s == -1) return "the compressed data ends inside a block";
            if (s < 0) return "invalid Huffman code";
            if (s < 256) {
                if (o >= cap) return "more data than ISIZE says";
                dst[o++] = (uint8_t)s;
                continue;
            }
            if (s == 256) break;
            s -= 257;
            if (s >= 29) return "invalid Huffman code (length symbol 286 or 287)";
            const int le = b.take(len_extra[s]);
            if (le < 0) return "the compressed data ends inside a block";
            const size_t ln = (size_t)len_base[s] + (size_t)le;
            const int ds = b.sym(*hd);
            if (ds == -1) return "the compressed data ends inside a block";
            if (ds < 0) return "invalid Huffman code";
            if (ds >= 30) return "invalid distance (symbol 30 or 31)";
            const int de = b.take(dist_extra[ds]);
            if (de < 0) return "the compressed data ends inside a block";
            const size_t d = (size_t)dist_base[ds] + (size_t)de;
            if (d > o) return "invalid distance (in front of the member's first byte)";
            if (ln > cap - o) return "more data than ISIZE says";
            for (size_t k = 0; k < ln; k++, o++) dst[o] = dst[o - d];       // (the ranges overlap when d < ln)
        }
    }
    out_len = o;
    return nullptr;
}

// ---- BGZF ------------------------------------------------------------------------------------------------------------
struct DgBgzfStats {
    size_t members = 0;
    uint64_t file_bytes = 0, inflated_bytes = 0;
    bool eof_member = false;
    unsigned threads = 1;
    double wall = 0, busy = 0;                              // seconds: the whole inflate; summed over the threads
};

// inflates a whole BGZF file into out; false with a message in err
inline bool dg_bgzf_inflate(const uint8_t *file, size_t size, unsigned threads, std::vector<uint8_t> &out, DgBgzfStats &st,
                            std::string &err) {
    struct Member { size_t at, cdata, clen; uint32_t crc, isize; uint64_t out; };
    std::vector<Member> ms;
    uint64_t total = 0;
    for (size_t p = 0; p < size;) {
        const std::string where = "BGZF member " + std::to_string(ms.size() + 1) + " (at byte " + std::to_string(p) + ")";
        if (size - p < 12) { err = where + ": the file ends inside a member's header (truncated)"; return false; }
        const uint8_t *h = file + p;
        if (h[0] != 31 || h[1] != 139 || h[2] != 8 || !(h[3] & 4)) { err = where + ": not a BGZF member (no gzip header with an extra field)"; return false; }
        const size_t xlen = h[10] | (size_t)h[11] << 8;
        if (size - p - 12 < xlen) { err = where + ": the file ends inside a member's header (truncated)"; return false; }
        size_t bsize = 0;
        for (size_t x = 0; x + 4 <= xlen;) {
            const uint8_t *e = h + 12 + x;
            const size_t sl = e[2] | (size_t)e[3] << 8;
            if (e[0] == 'B' && e[1] == 'C' && sl == 2 && x + 6 <= xlen) { bsize = (e[4] | (size_t)e[5] << 8) + 1; break; }
            x += 4 + sl;
        }
        if (!bsize) { err = where + ": no BC subfield in the gzip extra field (plain gzip, not BGZF?)"; return false; }
        if (bsize < 12 + xlen + 8) { err = where + ": BSIZE is smaller than the member's own header and trailer"; return false; }
        if (size - p < bsize) { err = where + ": the file ends inside the member (truncated: BSIZE says " + std::to_string(bsize) + " bytes, " + std::to_string(size - p) + " are left)"; return false; }
        const uint8_t *tr = h + bsize - 8;
        Member m;
        m.at = p; m.cdata = p + 12 + xlen; m.clen = bsize - 12 - xlen - 8;
        m.crc = tr[0] | (uint32_t)tr[1] << 8 | (uint32_t)tr[2] << 16 | (uint32_t)tr[3] << 24;
        m.isize = tr[4] | (uint32_t)tr[5] << 8 | (uint32_t)tr[6] << 16 | (uint32_t)tr[7] << 24;
        if (m.isize > 65536u) { err = where + ": ISIZE " + std::to_string(m.isize) + " is above the 64 KiB a BGZF member holds"; return false; }
        m.out = total; total += m.isize;
        ms.push_back(m);
        p += bsize;
    }
    out.resize(total);
    st.members = ms.size(); st.file_bytes = size; st.inflated_bytes = total;
    st.eof_member = !ms.empty() && ms.back().isize == 0;
    const unsigned nthr = (unsigned)std::max<size_t>(1, std::min<size_t>(threads, std::min<size_t>(64, ms.size())));
    st.threads = nthr;
    std::mutex mu;
    size_t bad = ms.size();                                 // the first member that failed, and why
    std::string why;
    double busy = 0;
    const auto t0 = std::chrono::steady_clock::now();
    auto work = [&](unsigned k) {
        const auto w0 = std::chrono::steady_clock::now();
        // runs of 16 members dealt round-robin: neighbours in the file stay with one thread
        for (size_t i0 = (size_t)k * 16; i0 < ms.size(); i0 += (size_t)nthr * 16)
            for (size_t i = i0; i < std::min(ms.size(), i0 + 16); i++) {
                const Member &m = ms[i];
                size_t got = 0;
                uint8_t *dst = out.data() + m.out;
                const char *e = dg_inflate(file + m.cdata, m.clen, dst, m.isize, got);
                std::string msg;
                if (e) msg = e;
                else if (got != m.isize) msg = "ISIZE says " + std::to_string(m.isize) + " bytes, the data inflates to " + std::to_string(got);
                else if (dg_crc32(dst, got) != m.crc) msg = "CRC32 mismatch";
                if (msg.empty()) continue;
                std::lock_guard<std::mutex> lk(mu);
                if (i < bad) { bad = i; why = "BGZF member " + std::to_string(i + 1) + " (at byte " + std::to_string(m.at) + "): " + msg; }
                return;
            }
        const double dt = std::chrono::duration<double>(std::chrono::steady_clock::now() - w0).count();
        std::lock_guard<std::mutex> lk(mu);
        busy += dt;
    };
    std::vector<std::thread> th;
    for (unsigned k = 1; k < nthr; k++) th.emplace_back(work, k);
    work(0);
    for (auto &x : th) x.join();
    st.wall = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    st.busy = busy;
    if (bad < ms.size()) { err = why; return false; }
    return true;
}

// ---- BAM -------------------------------------------------------------------------------------------------------------
struct DgBamRec {
    int32_t ref_id;
    uint32_t pos;                      // 1-based (BAM's pos + 1): SAM POS
    uint32_t flag;
    const char *name; uint32_t name_len;   // read_name without its NUL
    uint32_t l_seq;
    const uint8_t *seq;                // (l_seq + 1) / 2 bytes, two bases a byte, high nibble first
    const uint8_t *ops;                // n_ops little-endian 32-bit words, len << 4 | op (not aligned: memcpy)
    uint32_t n_ops;
    unsigned long long ordinal;        // 1-based, counting every record of the file
    const uint8_t *aux, *aux_end;      // the optional fields behind QUAL
};

// The one walker over a record's optional fields [t, end): the value of the first field tagged c0 c1 whose type is ty, or
// NULL (also when a field runs past the record).  ty 'Z' / 'H': the text, n its length without the NUL; ty 'B': the
// subtype byte (sub, when given, is the subtype asked for), then the 32-bit count, then the elements, n the count; any
// other type: the value, n its width.
inline const uint8_t *dg_bam_aux(const uint8_t *t, const uint8_t *end, char c0, char c1, uint8_t ty_want, size_t &n, uint8_t sub = 0) {
    auto width = [](uint8_t y) -> size_t { return y == 'c' || y == 'C' || y == 'A' ? 1 : y == 's' || y == 'S' ? 2 : y == 'i' || y == 'I' || y == 'f' ? 4 : 0; };
    while (end - t >= 3) {
        const bool hit = t[0] == (uint8_t)c0 && t[1] == (uint8_t)c1 && t[2] == ty_want;
        const uint8_t ty = t[2];
        t += 3;
        size_t sz = 0;
        if (ty == 'Z' || ty == 'H') {
            const void *z = memchr(t, 0, (size_t)(end - t));
            if (!z) return nullptr;
            sz = (size_t)((const uint8_t *)z - t) + 1;
            if (hit) { n = sz - 1; return t; }
        } else if (ty == 'B') {
            if (end - t < 5) return nullptr;
            const size_t w = width(t[0]);
            const uint64_t cnt = (uint32_t)(t[1] | (uint32_t)t[2] << 8 | (uint32_t)t[3] << 16 | (uint32_t)t[4] << 24);
            if (!w || cnt * w > (uint64_t)(end - t - 5)) return nullptr;
            if (hit && (!sub || t[0] == sub)) { n = (size_t)cnt; return t; }
            sz = 5 + (size_t)(cnt * w);
        } else {
            sz = width(ty);
            if (!sz || sz > (size_t)(end - t)) return nullptr;
            if (hit) { n = sz; return t; }
        }
        t += sz;
    }
    return nullptr;
}

// the letter of a 4-bit base code, for printing (--dump-parsed); the device decodes for itself (k_cigar.hip.h)
inline char dg_bam_base(const uint8_t *seq, uint32_t i) { return "=ACMGRSVTWYHKDBN"[(seq[i >> 1] >> ((~i & 1u) * 4u)) & 15u]; }

struct DgBamReader {
    struct Ref { std::string name; uint32_t len; };
    std::vector<uint8_t> u;            // the inflated file
    std::vector<Ref> refs;
    size_t at = 0;                     // the next record
    unsigned long long n_records = 0, n_skipped = 0;
    DgBgzfStats stats;

    static int32_t i32(const uint8_t *p) { return (int32_t)(p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24); }
    static uint32_t u32(const uint8_t *p) { return (uint32_t)i32(p); }

    // inflates the file and reads the header; false with a message in err
    bool open(const uint8_t *file, size_t size, unsigned threads, std::string &err) {
        if (!dg_bgzf_inflate(file, size, threads, u, stats, err)) return false;
        const size_t n = u.size();
        if (n < 4 || memcmp(u.data(), "BAM\1", 4) != 0) { err = "the input does not begin with the BAM magic (BAM\\1)"; return false; }
        if (n < 12) { err = "the BAM header runs past the end of the data"; return false; }
        const int64_t l_text = i32(&u[4]);
        if (l_text < 0 || (uint64_t)l_text > n - 12) { err = "the BAM header runs past the end of the data"; return false; }
        size_t p = 8 + (size_t)l_text;
        const int64_t n_ref = i32(&u[p]);
        p += 4;
        if (n_ref < 0) { err = "the BAM header has a negative number of references"; return false; }
        for (int64_t k = 0; k < n_ref; k++) {
            if (n - p < 4) { err = "the BAM header runs past the end of the data"; return false; }
            const int64_t ln = i32(&u[p]);
            p += 4;
            if (ln < 1 || (uint64_t)ln > n - p || n - p - (size_t)ln < 4) { err = "the BAM header runs past the end of the data"; return false; }
            Ref r;
            r.name.assign((const char *)&u[p], (size_t)ln - 1);
            r.len = u32(&u[p + (size_t)ln]);
            p += (size_t)ln + 4;
            refs.push_back(r);
        }
        at = p;
        return true;
    }

    // the next record that is not skipped: 1, 0 at the end of the data, -1 with a message in err.  Skipped as --sam
    // skips (counted in n_skipped): FLAG 0x4 or 0x100, refID < 0, no CIGAR ops, no SEQ.
    int next(DgBamRec &r, std::string &err) {
        for (;;) {
            const size_t n = u.size();
            if (at >= n) return 0;
            const unsigned long long ord = n_records + 1;
            const std::string where = "record " + std::to_string(ord);
            if (n - at < 4) { err = where + " runs past the end of the data (truncated)"; return -1; }
            const int64_t bs = i32(&u[at]);
            if (bs < 32) { err = where + ": block_size " + std::to_string(bs) + " is below a record's fixed part"; return -1; }
            if ((uint64_t)bs > n - at - 4) { err = where + " runs past the end of the data (truncated: block_size " + std::to_string(bs) + ", " + std::to_string(n - at - 4) + " bytes are left)"; return -1; }
            const uint8_t *b = &u[at + 4], *end = b + bs;
            n_records = ord;
            at += 4 + (size_t)bs;
            const uint32_t l_name = b[8], n_cig = b[12] | (uint32_t)b[13] << 8, flag = b[14] | (uint32_t)b[15] << 8;
            const int64_t l_seq = i32(b + 16);
            if (l_seq < 0) { err = where + ": negative l_seq"; return -1; }
            const uint64_t need = 32ull + l_name + 4ull * n_cig + ((uint64_t)l_seq + 1) / 2 + (uint64_t)l_seq;
            if (need > (uint64_t)bs) { err = where + ": its name, CIGAR, SEQ and QUAL do not fit its block_size"; return -1; }
            r.ref_id = i32(b); r.pos = u32(b + 4) + 1u; r.flag = flag;
            r.name = (const char *)b + 32; r.name_len = l_name ? l_name - 1 : 0;
            r.l_seq = (uint32_t)l_seq;
            r.ops = b + 32 + l_name; r.n_ops = n_cig;
            r.seq = r.ops + 4ull * n_cig;
            r.ordinal = ord;
            r.aux = b + need; r.aux_end = end;
            if ((flag & (0x4u | 0x100u)) || r.ref_id < 0 || n_cig == 0 || l_seq == 0) { n_skipped++; continue; }
            if ((uint64_t)r.ref_id >= refs.size()) { err = where + " (" + std::string(r.name, r.name_len) + "): refID " + std::to_string(r.ref_id) + " but the header has " + std::to_string(refs.size()) + " references"; return -1; }
            // more than 65,535 ops: <l_seq>S<ref_len>N in the record, the real ops in the CG:B,I tag
            if (n_cig == 2 && u32(r.ops) == (((uint32_t)l_seq << 4) | 4u) && (u32(r.ops + 4) & 15u) == 3u) {
                size_t cnt = 0;
                const uint8_t *cg = dg_bam_aux(r.aux, r.aux_end, 'C', 'G', 'B', cnt, 'I');
                const bool found = cg != nullptr;
                if (found) { r.ops = cg + 5; r.n_ops = (uint32_t)cnt; }
                if (!found || r.n_ops == 0) { err = where + " (" + std::string(r.name, r.name_len) + "): its CIGAR is the placeholder " + std::to_string(l_seq) + "S" + std::to_string(u32(b + 32 + l_name + 4) >> 4) + "N of a record with more than 65,535 ops, but it has no CG:B,I tag"; return -1; }
            }
            return 1;
        }
    }
};

// the header's references against --ref: a reference whose length differs from the --ref sequence of its name is an
// error, as an @SQ line with another LN is for --sam (a name --ref does not hold: nothing to compare, until a record names it)
inline bool dg_bam_check_refs(const DgBamReader &bam, const DgRefSeqs &ref, std::string &err) {
    for (const DgBamReader::Ref &r : bam.refs) {
        const DgRefSeqs::Span *sp = ref.find(r.name.data(), r.name.size());
        if (!sp || sp->len == r.len) continue;
        err = "BAM header: reference " + r.name + " has length " + std::to_string(r.len) + " but the --ref sequence of that name has " +
              std::to_string(sp->len) + " bases";
        return false;
    }
    return true;
}

// a record of the reader as the pipeline's record, the one place a DgBamRec becomes one: SEQ and the ops stay as they lie in the file
// (want_md: the md kinds look for the MD:Z field; a record without it is skipped by the caller)
inline void dg_bam_rec(const DgBamReader &bam, const DgBamRec &br, const DgRefSeqs &ref, DgAlnRec &r, bool want_md = false) {
    const std::string &rn = bam.refs[(size_t)br.ref_id].name;
    r = DgAlnRec{};
    r.rname = rn.data(); r.rname_len = (uint32_t)rn.size(); r.target = ref.find(rn.data(), rn.size());
    r.qname = br.name; r.qname_len = br.name_len;
    r.pos = br.pos;
    r.q = (const char *)br.seq; r.q_len = br.l_seq;
    r.bam_ops = br.ops; r.nops = br.n_ops;
    r.reverse = (br.flag & DG_SAM_REVERSE) != 0;
    r.where = br.ordinal;
    size_t n = 0;
    const uint8_t *md = want_md ? dg_bam_aux(br.aux, br.aux_end, 'M', 'D', 'Z', n) : nullptr;
    if (md) { r.md = (const char *)md; r.md_len = (uint32_t)n; }
}

// --md: the targets are the header's references, names and lengths only (ref.bases stays empty, a span's off is unused)
inline bool dg_bam_header_refs(const DgBamReader &bam, DgRefSeqs &ref, std::string &err) {
    for (const DgBamReader::Ref &r : bam.refs)
        if (!ref.by_name.emplace(r.name, DgRefSeqs::Span{0, r.len}).second) { err = "BAM header: reference " + r.name + " occurs twice"; return false; }
    return true;
}
