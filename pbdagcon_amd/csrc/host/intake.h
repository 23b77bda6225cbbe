// intake.h -- where the command-line hosts hand alignment records to the library: one description of a batch's arrays
// for every kind of input, one call that fills the library's struct and picks the entry point (whole targets or windows),
// and the text of the warning for a target or window that a record fails.
#pragma once
#include <cstdint>
#include <cstring>

#include "../../../include/dagcon.h"

enum DgRecordKind {
    DG_REC_PLAIN,       // --sam: one base a byte                          dagcon_consensus_cigar / _cigar_windows
    DG_REC_PACKED,      // --bam: two bases a byte                         dagcon_consensus_cigar_packed
    DG_REC_STRANDED,    // --paf: one base a byte, a flag per record       dagcon_consensus_cigar_strand
    DG_REC_CS           // --paf --cs: no bases, cs:Z: text per record     dagcon_consensus_cs
};

// the arrays of a batch: a dagcon_cigar_batch (DG_REC_CS: q_off / q_blob / q_bytes are the cs texts, op_begin / ops unused)
// and what the stranded and the cs kinds add to it
struct DgRecordArrays {
    dagcon_cigar_batch cb;
    const uint8_t *reverse;                                        // DG_REC_STRANDED
    const uint32_t *cs_len, *t_span;                               // DG_REC_CS
};

// windows NULL: whole targets
inline int dg_consensus_records(dagcon_ctx *ctx, DgRecordKind kind, const DgRecordArrays &a, const dagcon_windows *windows, dagcon_results *r) {
    const dagcon_cigar_batch &cb = a.cb;
    if (kind == DG_REC_CS) {
        dagcon_cs_batch sb;
        memset(&sb, 0, sizeof sb);
        sb.n_targets = cb.n_targets; sb.tlen = cb.tlen; sb.t_off = cb.t_off; sb.t_blob = cb.t_blob; sb.t_bytes = cb.t_bytes;
        sb.rec_begin = cb.rec_begin; sb.pos = cb.pos; sb.q_len = cb.q_len; sb.t_span = a.t_span;
        sb.cs_off = cb.q_off; sb.cs_len = a.cs_len; sb.cs_blob = cb.q_blob; sb.cs_bytes = cb.q_bytes;
        return dagcon_consensus_cs(ctx, &sb, windows, r);
    }
    return kind == DG_REC_PACKED ? dagcon_consensus_cigar_packed(ctx, &cb, windows, r)
         : kind == DG_REC_STRANDED ? dagcon_consensus_cigar_strand(ctx, &cb, windows, a.reverse, r)
         : windows ? dagcon_consensus_cigar_windows(ctx, &cb, windows, r) : dagcon_consensus_cigar(ctx, &cb, r);
}

// why DAGCON_ERR_NONCONFORMING came back for a target or a window of record input
inline const char *dg_nonconforming_text(bool cs_text) {
    return cs_text ? "a line's cs:Z: text breaks the grammar or does not fit its qe - qs, its te - ts or its target"
                   : "a record's CIGAR does not fit its SEQ or its target, or holds N or a length of 0";
}
