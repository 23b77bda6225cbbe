"""ctypes binding of the C ABI in include/dagcon.h (libdagcon_hip.so).

There is no fallback: if the HIP extension is missing or no GPU is present the
calls raise.  Nothing here imports oracle/.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libdagcon_hip.so")

DAGCON_OK = 0
ERR_NAMES = {
    -1: "DAGCON_ERR_INVALID_ARG", -2: "DAGCON_ERR_NO_DEVICE", -3: "DAGCON_ERR_HIP",
    -4: "DAGCON_ERR_NONCONFORMING", -5: "DAGCON_ERR_UNSUPPORTED", -6: "DAGCON_ERR_WORKSPACE",
    -7: "DAGCON_ERR_INTERNAL", -8: "DAGCON_ERR_STATE",
}
FLAG_RAW_ALIGNMENTS = 1
FLAG_STOP_AFTER_BUILD = 2
FLAG_STOP_AFTER_MERGE = 4
FLAG_DEBUG_RESWEEP = 16
FLAG_LOCAL_ALIGN = 32
FLAG_BASE_SUPPORT = 64
FLAG_BASE_POS = 256
MAX_COVERAGE = 4094
PLACE_MAX_LEN = 65536

EXPORTS = [
    "dagcon_abi_version", "dagcon_default_opts", "dagcon_create", "dagcon_destroy",
    "dagcon_last_error", "dagcon_consensus", "dagcon_upload", "dagcon_run", "dagcon_sync",
    "dagcon_fetch", "dagcon_get_timings", "dagcon_normalize", "dagcon_debug_graph",
    "dagcon_debug_counters", "dagcon_host_alloc", "dagcon_host_free", "dagcon_align",
    "dagcon_consensus_pre", "dagcon_debug_plan", "dagcon_align_dropped", "dagcon_align_panels",
    "dagcon_align_ends", "dagcon_place", "dagcon_fetch_support", "dagcon_upload_cigar", "dagcon_consensus_cigar",
    "dagcon_fetch_positions", "dagcon_upload_cigar_windows", "dagcon_consensus_cigar_windows",
    "dagcon_upload_cigar_packed", "dagcon_consensus_cigar_packed",
    "dagcon_upload_cigar_strand", "dagcon_consensus_cigar_strand",
    "dagcon_upload_cs", "dagcon_consensus_cs",
    "dagcon_set_record_filter", "dagcon_fetch_record_stats",
    "dagcon_set_edits", "dagcon_fetch_edits",
    "dagcon_set_edit_support", "dagcon_fetch_edit_support",
    "dagcon_set_pileup", "dagcon_fetch_pileup", "dagcon_fetch_pileup_sites",
    "dagcon_set_site_reads", "dagcon_fetch_site_reads",
    "dagcon_set_site_alleles", "dagcon_fetch_site_alleles", "dagcon_allele_text",
    "dagcon_set_site_join", "dagcon_fetch_joined_sites",
    "dagcon_set_hap_consensus", "dagcon_fetch_hap_tally", "dagcon_upload_haps", "dagcon_fetch_hap_map",
    "dagcon_upload_cigar_md", "dagcon_consensus_cigar_md", "dagcon_fetch_md_targets",
    "dagcon_set_window_phase", "dagcon_fetch_window_phase",
    "dagcon_set_hap_calls", "dagcon_fetch_hap_calls",
    "dagcon_upload_haps_swapped", "dagcon_set_window_keep", "dagcon_fetch_window_keep",
    "dagcon_set_site_link", "dagcon_fetch_site_link",
]
HC_NOCOVER, HC_HET, HC_CLASH, HC_HOM = 0, 1, 2, 3
HC_NONE = 0xFFFFFFFFFFFFFFFF
ABI_VERSION = 2


class DagconError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"{ERR_NAMES.get(code, code)}: {msg}")
        self.code = code


class Opts(C.Structure):
    _fields_ = [("min_cov", C.c_uint32), ("min_len", C.c_uint32), ("trim", C.c_uint32),
                ("min_weight", C.c_int32), ("device", C.c_int32), ("flags", C.c_uint32),
                ("max_segments", C.c_uint32), ("min_segment_len", C.c_uint32)]


class Batch(C.Structure):
    _fields_ = [("n_targets", C.c_uint32), ("tlen", C.c_void_p), ("aln_begin", C.c_void_p),
                ("aln_start", C.c_void_p), ("aln_off", C.c_void_p), ("aln_len", C.c_void_p),
                ("qstr", C.c_void_p), ("tstr", C.c_void_p), ("blob_bytes", C.c_uint64),
                ("backbone", C.c_void_p), ("backbone_off", C.c_void_p)]


class PreBatch(C.Structure):
    _fields_ = [("n_targets", C.c_uint32), ("tlen", C.c_void_p), ("rec_begin", C.c_void_p),
                ("tstart", C.c_void_p), ("strand", C.c_void_p), ("q_off", C.c_void_p), ("q_len", C.c_void_p),
                ("t_off", C.c_void_p), ("t_len", C.c_void_p), ("q_blob", C.c_void_p), ("q_bytes", C.c_uint64),
                ("t_blob", C.c_void_p), ("t_bytes", C.c_uint64)]


class CigarBatch(C.Structure):
    _fields_ = [("n_targets", C.c_uint32), ("tlen", C.c_void_p), ("t_off", C.c_void_p), ("t_blob", C.c_void_p),
                ("t_bytes", C.c_uint64), ("rec_begin", C.c_void_p), ("pos", C.c_void_p), ("q_off", C.c_void_p),
                ("q_len", C.c_void_p), ("q_blob", C.c_void_p), ("q_bytes", C.c_uint64), ("op_begin", C.c_void_p),
                ("ops", C.c_void_p)]


class CsBatch(C.Structure):
    _fields_ = [("n_targets", C.c_uint32), ("tlen", C.c_void_p), ("t_off", C.c_void_p), ("t_blob", C.c_void_p),
                ("t_bytes", C.c_uint64), ("rec_begin", C.c_void_p), ("pos", C.c_void_p), ("q_len", C.c_void_p),
                ("t_span", C.c_void_p), ("cs_off", C.c_void_p), ("cs_len", C.c_void_p), ("cs_blob", C.c_void_p),
                ("cs_bytes", C.c_uint64)]


class MdTags(C.Structure):
    """dagcon_md_tags: one MD:Z text per record of a dagcon_cigar_batch."""
    _fields_ = [("md_off", C.c_void_p), ("md_len", C.c_void_p), ("md_blob", C.c_void_p), ("md_bytes", C.c_uint64)]


class Windows(C.Structure):
    _fields_ = [("n_windows", C.c_uint32), ("target", C.c_void_p), ("begin", C.c_void_p), ("end", C.c_void_p)]


class Results(C.Structure):
    _fields_ = [("n_targets", C.c_uint32), ("n_segments", C.c_uint64),
                ("seg_begin", C.POINTER(C.c_uint64)), ("range0", C.POINTER(C.c_int32)),
                ("range1", C.POINTER(C.c_int32)), ("seq_off", C.POINTER(C.c_uint64)),
                ("seq_len", C.POINTER(C.c_uint32)), ("seq_blob", C.c_void_p),
                ("seq_bytes", C.c_uint64), ("target_status", C.POINTER(C.c_int32)),
                ("n_failed", C.c_uint32)]


class Support(C.Structure):
    _fields_ = [("n", C.c_uint64), ("weight", C.POINTER(C.c_uint16)), ("depth", C.POINTER(C.c_uint16))]


class RecordFilter(C.Structure):
    """dagcon_record_filter: max_error_ppm 1000000 keeps every record, max_depth 0 is off."""
    _fields_ = [("max_error_ppm", C.c_uint32), ("max_depth", C.c_uint32)]


class RecordStats(C.Structure):
    _fields_ = [("n", C.c_uint64), ("match", C.POINTER(C.c_uint32)), ("mismatch", C.POINTER(C.c_uint32)),
                ("ins", C.POINTER(C.c_uint32)), ("del_", C.POINTER(C.c_uint32)), ("fate", C.POINTER(C.c_uint8))]


FATE_MAX_ERROR, FATE_MAX_DEPTH, FATE_NONCONFORMING = 1, 2, 4


class EditSupport(C.Structure):
    """dagcon_edit_support: per edit its group's window and the alignments behind it (include/dagcon.h has the rule)."""
    _fields_ = [("n", C.c_uint64), ("w_begin", C.POINTER(C.c_uint32)), ("w_end", C.POINTER(C.c_uint32)),
                ("span", C.POINTER(C.c_uint32)), ("alt", C.POINTER(C.c_uint32)), ("ref", C.POINTER(C.c_uint32))]


class PileupOpts(C.Structure):
    """dagcon_pileup_opts: a position is a site when its second allele has at least min_count alignments and at least
    min_frac_ppm millionths of the depth (include/dagcon.h has the rule)."""
    _fields_ = [("min_count", C.c_uint32), ("min_frac_ppm", C.c_uint32)]


class Pileup(C.Structure):
    """dagcon_pileup: eight uint16 per position (A C G T N DEL INS 0), target t's from pos_begin[t]."""
    _fields_ = [("n_targets", C.c_uint32), ("pos_begin", C.POINTER(C.c_uint64)), ("counts", C.POINTER(C.c_uint16))]


class PileupSites(C.Structure):
    """dagcon_pileup_sites: target t's sites are [site_begin[t], site_begin[t + 1]), eight uint16 per site."""
    _fields_ = [("n_targets", C.c_uint32), ("site_begin", C.POINTER(C.c_uint64)), ("pos", C.POINTER(C.c_uint32)),
                ("counts", C.POINTER(C.c_uint16))]


class SiteReadsOpts(C.Structure):
    """dagcon_site_reads_opts: phase != 0 splits each target's alignments in two; rounds 0 is the default, 8 (include/dagcon.h
    has the rule)."""
    _fields_ = [("phase", C.c_uint32), ("rounds", C.c_uint32)]


class SiteReads(C.Structure):
    """dagcon_site_reads: the taken alignments, their entries at the sites of dagcon_pileup_sites, hap and phase."""
    _fields_ = [("n_aln", C.c_uint64), ("aln_tgt", C.POINTER(C.c_uint32)), ("aln_src", C.POINTER(C.c_uint64)),
                ("ent_begin", C.POINTER(C.c_uint64)), ("ent_site", C.POINTER(C.c_uint64)), ("ent_code", C.POINTER(C.c_uint8)),
                ("hap", C.POINTER(C.c_uint8)), ("phase", C.POINTER(C.c_int8))]


class SiteAlleles(C.Structure):
    """dagcon_site_alleles: per site of dagcon_pileup_sites its table of alleles (key, count, c1 c2 c0), per entry of
    dagcon_site_reads the index of its allele (include/dagcon.h has the rule)."""
    _fields_ = [("n_sites", C.c_uint64), ("al_begin", C.POINTER(C.c_uint64)), ("key", C.POINTER(C.c_uint64)),
                ("count", C.POINTER(C.c_uint32)), ("hap_count", C.POINTER(C.c_uint16)), ("n_ent", C.c_uint64),
                ("ent_allele", C.POINTER(C.c_uint16))]


class JoinedSites(C.Structure):
    """dagcon_joined_sites: the runs of adjacent sites of dagcon_pileup_sites, per run its spanning and partial members and
    its table of joined alleles (key, count, c1 c2 c0), per entry of dagcon_site_reads the index of its alignment's joined
    allele or 0xFFFF (include/dagcon.h has the rule, 10)."""
    _fields_ = [("n_runs", C.c_uint64), ("run_begin", C.POINTER(C.c_uint64)), ("spanning", C.POINTER(C.c_uint32)),
                ("partial", C.POINTER(C.c_uint32)), ("jal_begin", C.POINTER(C.c_uint64)), ("key", C.POINTER(C.c_uint64)),
                ("count", C.POINTER(C.c_uint32)), ("hap_count", C.POINTER(C.c_uint16)), ("n_ent", C.c_uint64),
                ("ent_joined", C.POINTER(C.c_uint16))]


class HapOpts(C.Structure):
    """dagcon_hap_opts: a target is split when it has at least min_sites separating sites and min_reads alignments of
    either label; 0, 0 are the defaults 2 and 3 (include/dagcon.h has the rule)."""
    _fields_ = [("min_sites", C.c_uint32), ("min_reads", C.c_uint32)]


class HapTally(C.Structure):
    """dagcon_hap_tally: per target n1, n2, n0, n_sep, agree, disagree and split; P1 M1 P2 M2 per site of dagcon_pileup_sites."""
    _fields_ = [("n_targets", C.c_uint32), ("n1", C.POINTER(C.c_uint32)), ("n2", C.POINTER(C.c_uint32)), ("n0", C.POINTER(C.c_uint32)),
                ("n_sep", C.POINTER(C.c_uint32)), ("agree", C.POINTER(C.c_uint32)), ("disagree", C.POINTER(C.c_uint32)),
                ("split", C.POINTER(C.c_uint8)), ("site_counts", C.POINTER(C.c_uint16))]


class WindowPhaseOpts(C.Structure):
    """dagcon_window_phase_opts: a window is linked to the one in front when max(same, diff) >= min_links, the two differ and
    the smaller is at most max_conflict_ppm of their sum; 0, 0 are the defaults 3 and 250000 (include/dagcon.h, rule 9)."""
    _fields_ = [("min_links", C.c_uint32), ("max_conflict_ppm", C.c_uint32)]


class WindowPhase(C.Structure):
    """dagcon_window_phase: per window same, diff, block and flip; the oriented hap per alignment of dagcon_site_reads and
    the oriented phase per site of dagcon_pileup_sites."""
    _fields_ = [("n_windows", C.c_uint32), ("same", C.POINTER(C.c_uint32)), ("diff", C.POINTER(C.c_uint32)),
                ("block", C.POINTER(C.c_uint32)), ("flip", C.POINTER(C.c_uint8)),
                ("n_aln", C.c_uint64), ("hap", C.POINTER(C.c_uint8)),
                ("n_sites", C.c_uint64), ("phase", C.POINTER(C.c_int8))]


class HapMap(C.Structure):
    """dagcon_hap_map: the targets of the batch dagcon_upload_haps derived, two per split target of the first batch."""
    _fields_ = [("n_targets", C.c_uint32), ("src_target", C.POINTER(C.c_uint32)), ("label", C.POINTER(C.c_uint8)),
                ("aln_begin", C.POINTER(C.c_uint64)), ("aln_src", C.POINTER(C.c_uint64))]


class HapCalls(C.Structure):
    _fields_ = [("n", C.c_uint64), ("state", C.POINTER(C.c_uint8)), ("mate", C.POINTER(C.c_uint64))]


class WindowKeepOpts(C.Structure):
    """dagcon_window_keep_opts: lo and hi per window of the first batch (include/dagcon.h, rule 12)."""
    _fields_ = [("n", C.c_uint32), ("lo", C.POINTER(C.c_uint32)), ("hi", C.POINTER(C.c_uint32))]


class WindowKeep(C.Structure):
    """dagcon_window_keep: per segment of the last results the kept part [i0, i1) and the positions of its two ends."""
    _fields_ = [("n_segments", C.c_uint64), ("i0", C.POINTER(C.c_uint32)), ("i1", C.POINTER(C.c_uint32)),
                ("p_first", C.POINTER(C.c_uint32)), ("p_last", C.POINTER(C.c_uint32))]


class SiteLinkOpts(C.Structure):
    """dagcon_site_link_opts: two sites are partners when at most max_conflict_ppm of the reads signed at both disagree and
    the smaller of the two agreeing cells holds min_cell reads; a site is linked with min_partners partners among the
    `reach` sites on either side; 0 in a field is its default: 100000, 3, 2, 256 (include/dagcon.h, rule 13)."""
    _fields_ = [("max_conflict_ppm", C.c_uint32), ("min_cell", C.c_uint32), ("min_partners", C.c_uint32), ("reach", C.c_uint32)]


class SiteLink(C.Structure):
    """dagcon_site_link: partners and linked per site of dagcon_pileup_sites."""
    _fields_ = [("n_sites", C.c_uint64), ("partners", C.POINTER(C.c_uint16)), ("linked", C.POINTER(C.c_uint8))]


class Edits(C.Structure):
    """dagcon_edits: per segment its target span and its edits (include/dagcon.h has the definition)."""
    _fields_ = [("n_segments", C.c_uint64), ("n", C.c_uint64), ("seg_t0", C.POINTER(C.c_uint32)),
                ("seg_t1", C.POINTER(C.c_uint32)), ("edit_begin", C.POINTER(C.c_uint64)),
                ("t_pos", C.POINTER(C.c_uint32)), ("t_len", C.POINTER(C.c_uint32)),
                ("c_off", C.POINTER(C.c_uint64)), ("c_len", C.POINTER(C.c_uint32))]


class Timings(C.Structure):
    _fields_ = [("ms_total", C.c_float), ("ms_normalize", C.c_float), ("ms_build", C.c_float),
                ("ms_merge", C.c_float), ("ms_bestpath", C.c_float),
                ("algorithmic_bytes", C.c_uint64), ("consensus_bases", C.c_uint64),
                ("n_alignments", C.c_uint64), ("n_columns", C.c_uint64), ("n_nodes", C.c_uint64),
                ("reruns", C.c_uint32), ("merge_segments", C.c_uint32)]


class GraphDump(C.Structure):
    _fields_ = [("n_nodes", C.c_uint32), ("base", C.POINTER(C.c_uint8)),
                ("weight", C.POINTER(C.c_int32)), ("coverage", C.POINTER(C.c_int32)),
                ("deleted", C.POINTER(C.c_uint8)), ("backbone", C.POINTER(C.c_uint8)),
                ("bbpos", C.POINTER(C.c_int32)), ("out_begin", C.POINTER(C.c_uint32)),
                ("out_dst", C.POINTER(C.c_int32)), ("out_count", C.POINTER(C.c_int32)),
                ("in_begin", C.POINTER(C.c_uint32)), ("in_src", C.POINTER(C.c_int32))]


_LIB = None


def load() -> C.CDLL:
    """Load libdagcon_hip.so; raises if it has not been built (no fallback)."""
    global _LIB
    if _LIB is not None:
        return _LIB
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950).  pbdagcon_amd has no CPU fallback.")
    L = C.CDLL(LIB_PATH)
    vp = C.c_void_p
    L.dagcon_abi_version.restype = C.c_int
    L.dagcon_default_opts.argtypes = [C.POINTER(Opts)]
    L.dagcon_create.argtypes = [C.POINTER(Opts), C.POINTER(vp)]
    L.dagcon_destroy.argtypes = [vp]
    L.dagcon_destroy.restype = None
    L.dagcon_last_error.argtypes = [vp]
    L.dagcon_last_error.restype = C.c_char_p
    L.dagcon_consensus.argtypes = [vp, C.POINTER(Batch), C.POINTER(Results)]
    L.dagcon_upload.argtypes = [vp, C.POINTER(Batch)]
    L.dagcon_run.argtypes = [vp]
    L.dagcon_sync.argtypes = [vp]
    L.dagcon_fetch.argtypes = [vp, C.POINTER(Results)]
    L.dagcon_get_timings.argtypes = [vp, C.POINTER(Timings)]
    L.dagcon_fetch_support.argtypes = [vp, C.POINTER(Support)]
    L.dagcon_normalize.argtypes = [vp, C.c_uint32, vp, vp, vp, vp, vp, C.c_uint64, C.c_uint32,
                                   C.c_uint32, vp, vp, vp, vp, vp]
    L.dagcon_debug_graph.argtypes = [vp, C.c_uint32, C.POINTER(GraphDump)]
    L.dagcon_align.argtypes = [vp, C.c_uint32, vp, vp, vp, vp, vp, C.c_uint64, vp, C.c_uint64, vp, vp, vp, vp]
    L.dagcon_align_panels.argtypes = [vp, C.c_uint32, vp, vp, vp, vp, vp, C.c_uint64, vp, C.c_uint64, vp, vp, vp,
                                      vp, vp, vp, vp, vp]
    L.dagcon_align_dropped.argtypes = [vp]
    L.dagcon_align_dropped.restype = C.c_uint32
    L.dagcon_align_ends.argtypes = [vp, C.c_uint32, vp, vp, vp, vp]
    L.dagcon_place.argtypes = [vp, vp, vp, vp, C.c_uint64, C.c_uint32, vp, vp, C.c_uint32, C.c_uint32,
                               vp, vp, vp, vp, vp]
    L.dagcon_upload_cigar.argtypes = [vp, C.POINTER(CigarBatch)]
    L.dagcon_consensus_cigar.argtypes = [vp, C.POINTER(CigarBatch), C.POINTER(Results)]
    L.dagcon_fetch_positions.argtypes = [vp, C.POINTER(C.POINTER(C.c_uint32)), C.POINTER(C.c_uint64)]
    L.dagcon_upload_cigar_windows.argtypes = [vp, C.POINTER(CigarBatch), C.POINTER(Windows)]
    L.dagcon_consensus_cigar_windows.argtypes = [vp, C.POINTER(CigarBatch), C.POINTER(Windows), C.POINTER(Results)]
    L.dagcon_upload_cigar_packed.argtypes = [vp, C.POINTER(CigarBatch), C.POINTER(Windows)]
    L.dagcon_consensus_cigar_packed.argtypes = [vp, C.POINTER(CigarBatch), C.POINTER(Windows), C.POINTER(Results)]
    L.dagcon_upload_cigar_strand.argtypes = [vp, C.POINTER(CigarBatch), C.POINTER(Windows), vp]
    L.dagcon_upload_cs.argtypes = [vp, C.POINTER(CsBatch), C.POINTER(Windows)]
    L.dagcon_consensus_cs.argtypes = [vp, C.POINTER(CsBatch), C.POINTER(Windows), C.POINTER(Results)]
    L.dagcon_consensus_cigar_strand.argtypes = [vp, C.POINTER(CigarBatch), C.POINTER(Windows), vp, C.POINTER(Results)]
    L.dagcon_set_record_filter.argtypes = [vp, C.POINTER(RecordFilter)]
    L.dagcon_fetch_record_stats.argtypes = [vp, C.POINTER(RecordStats)]
    L.dagcon_set_edits.argtypes = [vp, C.c_int]
    L.dagcon_fetch_edits.argtypes = [vp, C.POINTER(Edits)]
    L.dagcon_set_edit_support.argtypes = [vp, C.c_int]
    L.dagcon_fetch_edit_support.argtypes = [vp, C.POINTER(EditSupport)]
    L.dagcon_set_pileup.argtypes = [vp, C.POINTER(PileupOpts)]
    L.dagcon_fetch_pileup.argtypes = [vp, C.POINTER(Pileup)]
    L.dagcon_fetch_pileup_sites.argtypes = [vp, C.POINTER(PileupSites)]
    L.dagcon_set_site_reads.argtypes = [vp, C.POINTER(SiteReadsOpts)]
    L.dagcon_fetch_site_reads.argtypes = [vp, C.POINTER(SiteReads)]
    L.dagcon_set_site_alleles.argtypes = [vp, C.c_int]
    L.dagcon_fetch_site_alleles.argtypes = [vp, C.POINTER(SiteAlleles)]
    L.dagcon_set_site_join.argtypes = [vp, C.c_int]
    L.dagcon_fetch_joined_sites.argtypes = [vp, C.POINTER(JoinedSites)]
    L.dagcon_allele_text.argtypes = [C.c_uint64, C.c_char_p, C.c_size_t]
    L.dagcon_set_hap_consensus.argtypes = [vp, C.POINTER(HapOpts)]
    L.dagcon_fetch_hap_tally.argtypes = [vp, C.POINTER(HapTally)]
    L.dagcon_upload_haps.argtypes = [vp]
    L.dagcon_fetch_hap_map.argtypes = [vp, C.POINTER(HapMap)]
    L.dagcon_set_window_phase.argtypes = [vp, C.POINTER(WindowPhaseOpts)]
    L.dagcon_fetch_window_phase.argtypes = [vp, C.POINTER(WindowPhase)]
    L.dagcon_set_hap_calls.argtypes = [vp, C.c_int]
    L.dagcon_fetch_hap_calls.argtypes = [vp, C.POINTER(HapCalls)]
    L.dagcon_upload_haps_swapped.argtypes = [vp, vp]
    L.dagcon_set_window_keep.argtypes = [vp, C.POINTER(WindowKeepOpts)]
    L.dagcon_fetch_window_keep.argtypes = [vp, C.POINTER(WindowKeep)]
    L.dagcon_set_site_link.argtypes = [vp, C.POINTER(SiteLinkOpts)]
    L.dagcon_fetch_site_link.argtypes = [vp, C.POINTER(SiteLink)]
    L.dagcon_upload_cigar_md.argtypes = [vp, C.POINTER(CigarBatch), C.POINTER(Windows), C.POINTER(MdTags), C.c_int]
    L.dagcon_consensus_cigar_md.argtypes = [vp, C.POINTER(CigarBatch), C.POINTER(Windows), C.POINTER(MdTags), C.c_int,
                                            C.POINTER(Results)]
    L.dagcon_fetch_md_targets.argtypes = [vp, C.POINTER(vp), C.POINTER(C.c_uint64)]
    L.dagcon_host_alloc.argtypes = [vp, C.c_size_t, C.POINTER(vp)]
    L.dagcon_host_free.argtypes = [vp, vp]
    L.dagcon_host_free.restype = None
    _LIB = L
    return L


def allele_text(key) -> str:
    """dagcon_allele_text: the bases of an allele's key, "-" for the empty allele, a trailing "+" when it is long."""
    buf = C.create_string_buffer(24)
    r = load().dagcon_allele_text(int(key), buf, 24)
    if r != 0:
        raise DagconError(r, "dagcon_allele_text: %#x is no key" % int(key))
    return buf.value.decode()


def default_opts() -> Opts:
    o = Opts()
    load().dagcon_default_opts(C.byref(o))
    return o


class HostBatch:
    """numpy view of a dagcon_batch (structure-of-arrays blobs)."""

    def __init__(self, tlen, aln_begin, aln_start, aln_off, aln_len, qstr, tstr,
                 backbone=None, backbone_off=None, ids=None):
        self.tlen = np.ascontiguousarray(tlen, dtype=np.uint32)
        self.aln_begin = np.ascontiguousarray(aln_begin, dtype=np.uint64)
        self.aln_start = np.ascontiguousarray(aln_start, dtype=np.uint32)
        self.aln_off = np.ascontiguousarray(aln_off, dtype=np.uint64)
        self.aln_len = np.ascontiguousarray(aln_len, dtype=np.uint32)
        self.qstr = np.ascontiguousarray(np.frombuffer(qstr, dtype=np.uint8)
                                         if isinstance(qstr, (bytes, bytearray)) else qstr, dtype=np.uint8)
        self.tstr = np.ascontiguousarray(np.frombuffer(tstr, dtype=np.uint8)
                                         if isinstance(tstr, (bytes, bytearray)) else tstr, dtype=np.uint8)
        assert self.qstr.size == self.tstr.size
        self.backbone = None if backbone is None else np.ascontiguousarray(
            np.frombuffer(backbone, dtype=np.uint8) if isinstance(backbone, (bytes, bytearray)) else backbone,
            dtype=np.uint8)
        self.backbone_off = None if backbone_off is None else np.ascontiguousarray(backbone_off, dtype=np.uint64)
        self.ids = ids

    @property
    def n_targets(self):
        return int(self.tlen.size)

    @property
    def n_alns(self):
        return int(self.aln_len.size)

    def c_struct(self) -> Batch:
        b = Batch()
        b.n_targets = self.n_targets
        b.tlen = self.tlen.ctypes.data
        b.aln_begin = self.aln_begin.ctypes.data
        b.aln_start = self.aln_start.ctypes.data
        b.aln_off = self.aln_off.ctypes.data
        b.aln_len = self.aln_len.ctypes.data
        b.qstr = self.qstr.ctypes.data
        b.tstr = self.tstr.ctypes.data
        b.blob_bytes = self.qstr.size
        b.backbone = None if self.backbone is None else self.backbone.ctypes.data
        b.backbone_off = None if self.backbone_off is None else self.backbone_off.ctypes.data
        return b

    def target_alignments(self, t):
        """[(start, qstr, tstr)] of target t, as bytes."""
        out = []
        for a in range(int(self.aln_begin[t]), int(self.aln_begin[t + 1])):
            o, n = int(self.aln_off[a]), int(self.aln_len[a])
            out.append((int(self.aln_start[a]), self.qstr[o:o + n].tobytes(), self.tstr[o:o + n].tobytes()))
        return out

    def select(self, targets):
        """A new batch holding only the given targets (blobs are shared)."""
        targets = list(targets)
        begins = [0]
        idx = []
        for t in targets:
            a0, a1 = int(self.aln_begin[t]), int(self.aln_begin[t + 1])
            idx.extend(range(a0, a1))
            begins.append(len(idx))
        idx = np.asarray(idx, dtype=np.int64)
        return HostBatch(self.tlen[targets], begins, self.aln_start[idx], self.aln_off[idx],
                         self.aln_len[idx], self.qstr, self.tstr,
                         self.backbone, None if self.backbone_off is None else self.backbone_off[targets],
                         None if self.ids is None else [self.ids[t] for t in targets])


CIGAR_OPS = b"MIDNSHP=X"      # BAM op codes 0..8
BAM_NT16 = b"=ACMGRSVTWYHKDBN"     # BAM's 4-bit base codes 0..15


class HostCigarBatch:
    """numpy view of a dagcon_cigar_batch: per record a position, an ungapped read and BAM-encoded CIGAR ops
    (len << 4 | op), per target its bases once.  reverse (optional, one byte per record): the stranded calls
    (dagcon_upload_cigar_strand) -- q_blob holds the reads as the reads file has them and the device reads the bases of
    a record with reverse != 0 backwards and complemented.  t_blob None: a batch without target bases, for the MD calls
    (dagcon_upload_cigar_md), t_bytes the end of the last target."""

    def __init__(self, tlen, t_off, t_blob, rec_begin, pos, q_off, q_len, q_blob, op_begin, ops, ids=None, reverse=None):
        def u8(x):
            return np.ascontiguousarray(np.frombuffer(x, dtype=np.uint8) if isinstance(x, (bytes, bytearray)) else x,
                                        dtype=np.uint8)
        self.tlen = np.ascontiguousarray(tlen, dtype=np.uint32)
        self.t_off = np.ascontiguousarray(t_off, dtype=np.uint64)
        self.t_blob = None if t_blob is None else u8(t_blob)
        self.rec_begin = np.ascontiguousarray(rec_begin, dtype=np.uint64)
        self.pos = np.ascontiguousarray(pos, dtype=np.uint32)
        self.q_off = np.ascontiguousarray(q_off, dtype=np.uint64)
        self.q_len = np.ascontiguousarray(q_len, dtype=np.uint32)
        self.q_blob = u8(q_blob)
        self.op_begin = np.ascontiguousarray(op_begin, dtype=np.uint64)
        self.ops = np.ascontiguousarray(ops, dtype=np.uint32)
        self.ids = ids
        self.reverse = None if reverse is None else np.ascontiguousarray(np.asarray(reverse) != 0, dtype=np.uint8)
        if self.reverse is not None and self.reverse.shape != self.pos.shape:
            raise ValueError("reverse needs one entry per record")

    is_packed = False

    def packed(self) -> "HostCigarBatch":
        """The packed twin (dagcon_upload_cigar_packed): the reads in BAM's 4-bit encoding, two bases a byte, high
        nibble first, every record on a byte of its own.  A base outside =ACMGRSVTWYHKDBN (lower case too) raises
        ValueError."""
        if self.is_packed:
            return self
        if self.reverse is not None:
            raise ValueError("a batch with reverse has no packed form (dagcon_upload_cigar_strand takes one byte a base)")
        code = np.full(256, 255, dtype=np.uint8)
        code[np.frombuffer(BAM_NT16, dtype=np.uint8)] = np.arange(16, dtype=np.uint8)
        n = self.q_len.astype(np.int64)
        nb = (n + 1) // 2
        p_off = np.zeros(n.size, dtype=np.uint64)
        if n.size:
            p_off[1:] = np.cumsum(nb)[:-1]
        # nibble slots of the packed blob, two a byte; the slot of base i of record r is 2 * p_off[r] + i
        rec = np.repeat(np.arange(n.size), n)
        i = np.arange(int(n.sum()), dtype=np.int64) - np.repeat(np.cumsum(n) - n, n)
        src = self.q_blob[self.q_off.astype(np.int64)[rec] + i]
        c = code[src]
        if (c == 255).any():
            bad = int(src[c == 255][0])
            raise ValueError(f"read base {bytes([bad])!r} is not one of {BAM_NT16.decode()}")
        slots = np.zeros(2 * int(nb.sum()), dtype=np.uint8)
        slots[2 * p_off.astype(np.int64)[rec] + i] = c
        blob = (slots[0::2] << 4) | slots[1::2]
        out = HostCigarBatch(self.tlen, self.t_off, self.t_blob, self.rec_begin, self.pos, p_off, self.q_len, blob,
                             self.op_begin, self.ops, self.ids)
        out.is_packed = True
        return out

    @classmethod
    def from_records(cls, targets, ids=None):
        """targets = [(target bases, [(pos, read bases, [(op char or code, length)])])]."""
        tlen, t_off, rec_begin, pos, q_off, q_len, op_begin, ops = [], [], [0], [], [], [], [0], []
        tb, qb = [], []
        tp = qp = 0
        for tseq, recs in targets:
            tlen.append(len(tseq)); t_off.append(tp); tb.append(tseq); tp += len(tseq)
            for ps, q, cig in recs:
                pos.append(ps); q_off.append(qp); q_len.append(len(q)); qb.append(q); qp += len(q)
                for op, ln in cig:
                    code = op if isinstance(op, int) else CIGAR_OPS.index(op.encode() if isinstance(op, str) else op)
                    ops.append((int(ln) << 4) | code)
                op_begin.append(len(ops))
            rec_begin.append(len(pos))
        return cls(tlen, t_off, b"".join(tb), rec_begin, pos, q_off, q_len, b"".join(qb), op_begin, ops, ids)

    @property
    def n_targets(self):
        return int(self.tlen.size)

    @property
    def n_records(self):
        return int(self.pos.size)

    @property
    def t_bytes(self):
        if self.t_blob is not None:
            return int(self.t_blob.size)
        return int((self.t_off + self.tlen).max()) if self.tlen.size else 0

    @property
    def nbytes(self):
        """Bytes the call carries to the device: both blobs, the ops and the per-record / per-target arrays."""
        return int(sum(a.nbytes for a in (self.tlen, self.t_off, self.t_blob, self.rec_begin, self.pos, self.q_off,
                                          self.q_len, self.q_blob, self.op_begin, self.ops) if a is not None))

    def c_struct(self) -> CigarBatch:
        b = CigarBatch()
        b.n_targets = self.n_targets
        b.tlen = self.tlen.ctypes.data
        b.t_off = self.t_off.ctypes.data
        b.t_blob = None if self.t_blob is None else self.t_blob.ctypes.data
        b.t_bytes = self.t_bytes
        b.rec_begin = self.rec_begin.ctypes.data
        b.pos = self.pos.ctypes.data
        b.q_off = self.q_off.ctypes.data
        b.q_len = self.q_len.ctypes.data
        b.q_blob = self.q_blob.ctypes.data
        b.q_bytes = self.q_blob.size
        b.op_begin = self.op_begin.ctypes.data
        b.ops = self.ops.ctypes.data
        return b


class HostCsBatch:
    """numpy view of a dagcon_cs_batch: per record a position, the read and target lengths it claims and the text
    behind a PAF line's cs:Z: tag as the file has it, per target its bases once.  There are no read bases: the device
    decodes the text against the target (dagcon_upload_cs)."""

    def __init__(self, tlen, t_off, t_blob, rec_begin, pos, q_len, cs_off, cs_len, cs_blob, t_span=None, ids=None):
        def u8(x):
            return np.ascontiguousarray(np.frombuffer(x, dtype=np.uint8) if isinstance(x, (bytes, bytearray)) else x,
                                        dtype=np.uint8)
        self.tlen = np.ascontiguousarray(tlen, dtype=np.uint32)
        self.t_off = np.ascontiguousarray(t_off, dtype=np.uint64)
        self.t_blob = u8(t_blob)
        self.rec_begin = np.ascontiguousarray(rec_begin, dtype=np.uint64)
        self.pos = np.ascontiguousarray(pos, dtype=np.uint32)
        self.q_len = np.ascontiguousarray(q_len, dtype=np.uint32)
        self.cs_off = np.ascontiguousarray(cs_off, dtype=np.uint64)
        self.cs_len = np.ascontiguousarray(cs_len, dtype=np.uint32)
        self.cs_blob = u8(cs_blob)
        self.t_span = None if t_span is None else np.ascontiguousarray(t_span, dtype=np.uint32)
        self.ids = ids
        if self.t_span is not None and self.t_span.shape != self.pos.shape:
            raise ValueError("t_span needs one entry per record")

    @classmethod
    def from_records(cls, targets, with_span=True, ids=None):
        """targets = [(target bases, [(pos, q_len, t_span, cs text)])]."""
        tlen, t_off, rec_begin, pos, q_len, t_span, cs_off, cs_len = [], [], [0], [], [], [], [], []
        tb, cb = [], []
        tp = cp = 0
        for tseq, recs in targets:
            tlen.append(len(tseq)); t_off.append(tp); tb.append(tseq); tp += len(tseq)
            for ps, ql, ts, cs in recs:
                cs = cs.encode() if isinstance(cs, str) else cs
                pos.append(ps); q_len.append(ql); t_span.append(ts); cs_off.append(cp); cs_len.append(len(cs))
                cb.append(cs); cp += len(cs)
            rec_begin.append(len(pos))
        return cls(tlen, t_off, b"".join(tb), rec_begin, pos, q_len, cs_off, cs_len, b"".join(cb),
                   t_span if with_span else None, ids)

    @property
    def n_targets(self):
        return int(self.tlen.size)

    @property
    def n_records(self):
        return int(self.pos.size)

    @property
    def nbytes(self):
        """Bytes the call carries to the device: the text, the targets and the per-record / per-target arrays."""
        arrs = [self.tlen, self.t_off, self.t_blob, self.rec_begin, self.pos, self.q_len, self.cs_off, self.cs_len, self.cs_blob]
        return int(sum(a.nbytes for a in arrs) + (self.t_span.nbytes if self.t_span is not None else 0))

    def c_struct(self) -> CsBatch:
        b = CsBatch()
        b.n_targets = self.n_targets
        b.tlen = self.tlen.ctypes.data
        b.t_off = self.t_off.ctypes.data
        b.t_blob = self.t_blob.ctypes.data
        b.t_bytes = self.t_blob.size
        b.rec_begin = self.rec_begin.ctypes.data
        b.pos = self.pos.ctypes.data
        b.q_len = self.q_len.ctypes.data
        b.t_span = None if self.t_span is None else self.t_span.ctypes.data
        b.cs_off = self.cs_off.ctypes.data
        b.cs_len = self.cs_len.ctypes.data
        b.cs_blob = self.cs_blob.ctypes.data
        b.cs_bytes = self.cs_blob.size
        return b


class HostMdTags:
    """numpy view of a dagcon_md_tags: the text behind each record's MD:Z: tag as the file has it, back to back."""

    def __init__(self, md_off, md_len, md_blob):
        self.md_off = np.ascontiguousarray(md_off, dtype=np.uint64)
        self.md_len = np.ascontiguousarray(md_len, dtype=np.uint32)
        self.md_blob = np.ascontiguousarray(np.frombuffer(md_blob, dtype=np.uint8)
                                            if isinstance(md_blob, (bytes, bytearray)) else md_blob, dtype=np.uint8)
        if self.md_off.shape != self.md_len.shape:
            raise ValueError("md_off and md_len need one entry per record")

    @classmethod
    def from_texts(cls, texts):
        """texts: one bytes / str per record, in record order."""
        texts = [t.encode() if isinstance(t, str) else bytes(t) for t in texts]
        ln = np.asarray([len(t) for t in texts], dtype=np.uint32)
        off = np.zeros(len(texts), dtype=np.uint64)
        if len(texts):
            off[1:] = np.cumsum(ln.astype(np.uint64))[:-1]
        return cls(off, ln, b"".join(texts))

    @property
    def n_records(self):
        return int(self.md_off.size)

    @property
    def nbytes(self):
        return int(self.md_off.nbytes + self.md_len.nbytes + self.md_blob.nbytes)

    def c_struct(self) -> MdTags:
        m = MdTags()
        m.md_off, m.md_len, m.md_blob = self.md_off.ctypes.data, self.md_len.ctypes.data, self.md_blob.ctypes.data
        m.md_bytes = self.md_blob.size
        return m


class HostWindows:
    """numpy view of a dagcon_windows: per window its target (index into the cigar batch) and [begin, end) in target
    bases; targets ascending, begins ascending inside a target, windows may overlap."""

    def __init__(self, target, begin, end):
        self.target = np.ascontiguousarray(target, dtype=np.uint32)
        self.begin = np.ascontiguousarray(begin, dtype=np.uint32)
        self.end = np.ascontiguousarray(end, dtype=np.uint32)
        if not (self.target.size == self.begin.size == self.end.size):
            raise ValueError("target, begin and end must have one entry per window")

    @classmethod
    def tiled(cls, tlens, window, overlap=0):
        """Window i of a target has the core [i W, min((i + 1) W, tlen)) and runs as the core widened by `overlap`
        on both sides, clipped to the target (what pbdagcon --sam --window does)."""
        tg, bg, en = [], [], []
        for g, tl in enumerate(tlens):
            tl = int(tl)
            for i in range(max(1, -(-tl // window)) if tl else 0):
                tg.append(g); bg.append(max(0, i * window - overlap)); en.append(min(tl, (i + 1) * window + overlap))
        return cls(tg, bg, en)

    @property
    def n_windows(self):
        return int(self.target.size)

    def c_struct(self) -> Windows:
        w = Windows()
        w.n_windows = self.n_windows
        w.target, w.begin, w.end = self.target.ctypes.data, self.begin.ctypes.data, self.end.ctypes.data
        return w


class Context:
    """dagcon_ctx handle.  One per GPU; single-owner."""

    def __init__(self, min_cov=6, min_len=500, trim=50, min_weight=-1, device=0, flags=0, max_segments=0,
                 min_segment_len=0):
        self.L = load()
        o = Opts()
        o.min_cov, o.min_len, o.trim, o.min_weight = min_cov, min_len, trim, min_weight
        o.device, o.flags, o.max_segments = device, flags, max_segments
        o.min_segment_len = min_segment_len
        self.opts = o
        self.h = C.c_void_p()
        rc = self.L.dagcon_create(C.byref(o), C.byref(self.h))
        if rc != DAGCON_OK:
            raise DagconError(rc, "dagcon_create failed (is a gfx950 GPU visible?)")
        self._keep = None
        self._pinned = []
        self.target_status = None      # per-target dagcon_status of the last fetch (ABI 2)
        self._align_n = 0              # pairs of the last align / consensus_pre (align_ends)
        self._segs = None              # (seg_begin, seq_off, seq_len) of the last results (base_support)

    def close(self):
        if getattr(self, "h", None) and self.h.value:
            for p in self._pinned:
                self.L.dagcon_host_free(self.h, p)
            self._pinned = []
            self.L.dagcon_destroy(self.h)
            self.h = C.c_void_p()

    def host_array(self, nbytes):
        """uint8 numpy array over page-locked host memory (dagcon_host_alloc); freed by close()."""
        p = C.c_void_p()
        self._chk(self.L.dagcon_host_alloc(self.h, max(int(nbytes), 1), C.byref(p)))
        self._pinned.append(p)
        return np.ctypeslib.as_array((C.c_uint8 * max(int(nbytes), 1)).from_address(p.value))[:int(nbytes)]

    def pin_batch(self, batch: "HostBatch") -> "HostBatch":
        """A copy of the batch whose string blobs live in page-locked memory."""
        q = self.host_array(batch.qstr.size); q[:] = batch.qstr
        t = self.host_array(batch.tstr.size); t[:] = batch.tstr
        bb = None
        if batch.backbone is not None:
            bb = self.host_array(batch.backbone.size); bb[:] = batch.backbone
        return HostBatch(batch.tlen, batch.aln_begin, batch.aln_start, batch.aln_off, batch.aln_len, q, t,
                         bb, batch.backbone_off, batch.ids)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc != DAGCON_OK:
            raise DagconError(rc, (self.L.dagcon_last_error(self.h) or b"").decode())

    def upload(self, batch: HostBatch):
        self._keep = batch
        b = batch.c_struct()
        self._chk(self.L.dagcon_upload(self.h, C.byref(b)))

    def run(self):
        self._chk(self.L.dagcon_run(self.h))

    def sync(self):
        self._chk(self.L.dagcon_sync(self.h))

    def _status(self, r, strict):
        """ABI 2: a failure is confined to its target.  strict (the default) raises for the first failed
        target, as a caller that cannot use a partial batch wants; strict=False returns the batch with
        [] for the failed targets and leaves their codes in self.target_status."""
        self.target_status = np.ctypeslib.as_array(r.target_status, shape=(r.n_targets,)).copy() if r.n_targets else np.zeros(0, np.int32)
        if strict and r.n_failed:
            t = int(np.flatnonzero(self.target_status)[0])
            raise DagconError(int(self.target_status[t]), (self.L.dagcon_last_error(self.h) or b"").decode())

    def fetch(self, strict=True):
        r = Results()
        self._chk(self.L.dagcon_fetch(self.h, C.byref(r)))
        out = self._keep_segs(r)
        self._status(r, strict)
        return out

    def _keep_segs(self, r):
        """_results_to_py, remembering where each segment's bases are (base_support)."""
        S = int(r.n_segments)
        self._segs = (np.ctypeslib.as_array(r.seg_begin, shape=(r.n_targets + 1,)).copy(),
                      np.ctypeslib.as_array(r.seq_off, shape=(S,)).copy() if S else np.zeros(0, np.uint64),
                      np.ctypeslib.as_array(r.seq_len, shape=(S,)).copy() if S else np.zeros(0, np.uint32))
        return _results_to_py(r)

    def fetch_support_raw(self):
        """dagcon_fetch_support: (weight, depth) uint16 arrays over the whole seq_blob of the last results (copies)."""
        s = Support()
        self._chk(self.L.dagcon_fetch_support(self.h, C.byref(s)))
        n = int(s.n)
        if n == 0:
            return np.zeros(0, np.uint16), np.zeros(0, np.uint16)
        return np.ctypeslib.as_array(s.weight, shape=(n,)).copy(), np.ctypeslib.as_array(s.depth, shape=(n,)).copy()

    def base_support(self):
        """Per target, one (weight, depth) pair of uint16 arrays per segment, aligned with that segment's seq
        (FLAG_BASE_SUPPORT; after consensus, fetch or consensus_pre).  weight: the node weight of the best-path vertex
        the base comes from; depth: the coverage of its backbone vertex (include/dagcon.h, dagcon_support)."""
        w, d = self.fetch_support_raw()
        sb, so, sl = self._segs
        out = []
        for t in range(sb.size - 1):
            out.append([(w[int(so[s]):int(so[s]) + int(sl[s])], d[int(so[s]):int(so[s]) + int(sl[s])])
                        for s in range(int(sb[t]), int(sb[t + 1]))])
        return out

    def fetch_positions_raw(self):
        """dagcon_fetch_positions: a uint32 array over the whole seq_blob of the last results (a copy)."""
        ptr, n = C.POINTER(C.c_uint32)(), C.c_uint64()
        self._chk(self.L.dagcon_fetch_positions(self.h, C.byref(ptr), C.byref(n)))
        if n.value == 0:
            return np.zeros(0, np.uint32)
        return np.ctypeslib.as_array(ptr, shape=(int(n.value),)).copy()

    def base_positions(self):
        """Per target, one uint32 array per segment, aligned with that segment's seq (FLAG_BASE_POS; after consensus,
        fetch or consensus_pre): _bbMap of the best-path vertex each base comes from -- target base p for a backbone
        vertex, the next target base for an inserted one (include/dagcon.h, dagcon_fetch_positions)."""
        pos = self.fetch_positions_raw()
        sb, so, sl = self._segs
        return [[pos[int(so[s]):int(so[s]) + int(sl[s])] for s in range(int(sb[t]), int(sb[t + 1]))]
                for t in range(sb.size - 1)]

    def fetch_raw(self):
        """dagcon_fetch without the conversion to Python objects: the returned struct points into
        host memory the context owns until its next fetch (dagcon_run does not touch it), so a
        caller can start the next run first and convert (results_to_py) meanwhile."""
        r = Results()
        self._chk(self.L.dagcon_fetch(self.h, C.byref(r)))
        self._status(r, True)
        return r

    results_to_py = staticmethod(lambda r: _results_to_py(r))

    def consensus(self, batch: HostBatch, strict=True):
        """Per target: [(range0, range1, seq_bytes)]."""
        self._keep = batch
        b = batch.c_struct()
        r = Results()
        self._chk(self.L.dagcon_consensus(self.h, C.byref(b), C.byref(r)))
        out = self._keep_segs(r)
        self._status(r, strict)
        return out

    def _intake(self, batch, windows, keep, consensus, strict=True):
        """The one way into the record intake.  The entry point follows from the batch (cs text; CIGAR records stranded,
        packed or plain), from windows (None: whole targets) and from consensus (False: upload only, then run / sync /
        fetch as after upload; True: the results, per target or per window [(range0, range1, seq_bytes)])."""
        self._keep = keep
        b = batch.c_struct()
        w = windows.c_struct() if windows is not None else None
        args = [self.h, C.byref(b), C.byref(w) if w is not None else None]
        if isinstance(batch, HostCsBatch):
            kind = "cs"
        elif batch.reverse is not None:
            kind = "cigar_strand"
            args.append(batch.reverse.ctypes.data)
        elif batch.is_packed:
            kind = "cigar_packed"
        elif w is not None:
            kind = "cigar_windows"
        else:
            kind = "cigar"
            args.pop()                 # (the one entry point without a windows parameter)
        if not consensus:
            self._chk(getattr(self.L, "dagcon_upload_" + kind)(*args))
            return None
        r = Results()
        self._chk(getattr(self.L, "dagcon_consensus_" + kind)(*args, C.byref(r)))
        out = self._keep_segs(r)
        self._status(r, strict)
        return out

    def upload_cigar(self, batch: HostCigarBatch):
        """dagcon_upload_cigar: then run / sync / fetch as after upload."""
        self._intake(batch, None, batch, False)

    def consensus_cigar(self, batch: HostCigarBatch, strict=True):
        """Per target: [(range0, range1, seq_bytes)], from (position, read, CIGAR) records expanded on the device."""
        return self._intake(batch, None, batch, True, strict)

    def upload_cigar_windows(self, batch: HostCigarBatch, windows: HostWindows):
        """dagcon_upload_cigar_windows: then run / sync / fetch as after upload (one result target per window)."""
        self._intake(batch, windows, (batch, windows), False)

    def consensus_cigar_windows(self, batch: HostCigarBatch, windows: HostWindows, strict=True):
        """Per window: [(range0, range1, seq_bytes)], the records cut to the windows on the device."""
        return self._intake(batch, windows, (batch, windows), True, strict)

    def upload_cs(self, batch: HostCsBatch, windows: HostWindows = None):
        """dagcon_upload_cs: then run / sync / fetch as after upload (with windows: one result target per window)."""
        self._intake(batch, windows, (batch, windows), False)

    def consensus_cs(self, batch: HostCsBatch, windows: HostWindows = None, strict=True):
        """Per target (per window with windows): [(range0, range1, seq_bytes)], from cs:Z: text decoded on the device."""
        return self._intake(batch, windows, (batch, windows), True, strict)

    def _intake_md(self, batch, md, windows, consensus, strict=True):
        self._keep = (batch, md, windows)
        b = batch.c_struct()
        m = md.c_struct() if md is not None else None
        w = windows.c_struct() if windows is not None else None
        args = [self.h, C.byref(b), C.byref(w) if w is not None else None, C.byref(m) if m is not None else None,
                1 if batch.is_packed else 0]
        if not consensus:
            self._chk(self.L.dagcon_upload_cigar_md(*args))
            return None
        r = Results()
        self._chk(self.L.dagcon_consensus_cigar_md(*args, C.byref(r)))
        out = self._keep_segs(r)
        self._status(r, strict)
        return out

    def upload_cigar_md(self, batch: HostCigarBatch, md: "HostMdTags", windows: HostWindows = None):
        """dagcon_upload_cigar_md: then run / sync / fetch as after upload.  batch.t_blob is not read (None is fine);
        a HostCigarBatch.packed() batch selects the packed form."""
        self._intake_md(batch, md, windows, False)

    def consensus_cigar_md(self, batch: HostCigarBatch, md: "HostMdTags", windows: HostWindows = None, strict=True):
        """Per target (per window with windows): [(range0, range1, seq_bytes)], the targets rebuilt on the device from
        the records' MD:Z texts."""
        return self._intake_md(batch, md, windows, True, strict)

    def md_targets(self):
        """dagcon_fetch_md_targets: the target blob the last upload_cigar_md / consensus_cigar_md rebuilt, a uint8 array
        of t_bytes bytes (a copy)."""
        ptr, n = C.c_void_p(), C.c_uint64()
        self._chk(self.L.dagcon_fetch_md_targets(self.h, C.byref(ptr), C.byref(n)))
        if n.value == 0:
            return np.zeros(0, np.uint8)
        return np.ctypeslib.as_array((C.c_uint8 * int(n.value)).from_address(ptr.value)).copy()

    def set_record_filter(self, max_error_ppm=1000000, max_depth=0):
        """dagcon_set_record_filter for every later record call (CIGAR, packed, stranded, cs; whole targets and windows):
        records above max_error_ppm are left out, then at most max_depth per target or window stay (include/dagcon.h
        has the rule).  The defaults leave nothing out and only make record_stats available; None for both: off."""
        if max_error_ppm is None and max_depth is None:
            self._chk(self.L.dagcon_set_record_filter(self.h, None))
            return
        f = RecordFilter(max_error_ppm, max_depth)
        self._chk(self.L.dagcon_set_record_filter(self.h, C.byref(f)))

    def record_stats(self) -> dict:
        """dagcon_fetch_record_stats: match, mismatch, ins, del (uint32) and fate (uint8, FATE_* bits), one entry per
        record of the last record upload under a filter (copies)."""
        st = RecordStats()
        self._chk(self.L.dagcon_fetch_record_stats(self.h, C.byref(st)))
        n = int(st.n)

        def arr(ptr, dt):
            return np.ctypeslib.as_array(ptr, shape=(n,)).copy() if n else np.zeros(0, dt)
        return {"match": arr(st.match, np.uint32), "mismatch": arr(st.mismatch, np.uint32), "ins": arr(st.ins, np.uint32),
                "del": arr(st.del_, np.uint32), "fate": arr(st.fate, np.uint8)}

    def set_edits(self, on=True):
        """dagcon_set_edits for every later record call (a FLAG_BASE_POS context): the device lists where each segment
        differs from its target (edits())."""
        self._chk(self.L.dagcon_set_edits(self.h, 1 if on else 0))

    def set_edit_support(self, on=True):
        """dagcon_set_edit_support for every later record call (set_edits must be on): the device counts, per edit, the
        alignments that span its window and those that carry the consensus' or the target's allele (edit_support())."""
        self._chk(self.L.dagcon_set_edit_support(self.h, 1 if on else 0))

    def edit_support(self) -> dict:
        """dagcon_fetch_edit_support (copies): w_begin, w_end, span, alt, ref (uint32, one per edit of edits())."""
        e = EditSupport()
        self._chk(self.L.dagcon_fetch_edit_support(self.h, C.byref(e)))
        n = int(e.n)
        return {k: (np.ctypeslib.as_array(getattr(e, k), shape=(n,)).copy() if n else np.zeros(0, np.uint32))
                for k in ("w_begin", "w_end", "span", "alt", "ref")}

    def set_pileup(self, min_count=0, min_frac_ppm=0):
        """dagcon_set_pileup for every later upload, whatever its kind: the device counts per target position what the
        alignments show there (pileup()) and lists the positions whose second allele has at least min_count alignments
        and min_frac_ppm millionths of the depth (pileup_sites()).  set_pileup(None): off."""
        if min_count is None:
            self._chk(self.L.dagcon_set_pileup(self.h, None))
            return
        o = PileupOpts(min_count, min_frac_ppm)
        self._chk(self.L.dagcon_set_pileup(self.h, C.byref(o)))

    def pileup(self) -> dict:
        """dagcon_fetch_pileup (copies): pos_begin (uint64, one per target and one more) and counts (uint16,
        [positions, 8]: A C G T N DEL INS 0; target t's rows are pos_begin[t] .. pos_begin[t + 1])."""
        pu = Pileup()
        self._chk(self.L.dagcon_fetch_pileup(self.h, C.byref(pu)))
        T = int(pu.n_targets)
        begin = np.ctypeslib.as_array(pu.pos_begin, shape=(T + 1,)).copy()
        n = int(begin[T])
        counts = np.ctypeslib.as_array(pu.counts, shape=(n, 8)).copy() if n else np.zeros((0, 8), np.uint16)
        return {"pos_begin": begin, "counts": counts}

    def pileup_sites(self) -> dict:
        """dagcon_fetch_pileup_sites (copies): site_begin (uint64, one per target and one more), pos (uint32, per site,
        relative to its target) and counts (uint16, [sites, 8])."""
        ps = PileupSites()
        self._chk(self.L.dagcon_fetch_pileup_sites(self.h, C.byref(ps)))
        T = int(ps.n_targets)
        begin = np.ctypeslib.as_array(ps.site_begin, shape=(T + 1,)).copy()
        n = int(begin[T])
        return {"site_begin": begin,
                "pos": np.ctypeslib.as_array(ps.pos, shape=(n,)).copy() if n else np.zeros(0, np.uint32),
                "counts": np.ctypeslib.as_array(ps.counts, shape=(n, 8)).copy() if n else np.zeros((0, 8), np.uint16)}

    def set_site_reads(self, phase=False, rounds=0):
        """dagcon_set_site_reads for every later upload made with set_pileup on: the device lists per taken alignment what
        it shows at each site (site_reads()); phase: it also splits each target's alignments in two, in `rounds` rounds
        (0: the default, 8).  set_site_reads(None): off."""
        if phase is None:
            self._chk(self.L.dagcon_set_site_reads(self.h, None))
            return
        o = SiteReadsOpts(1 if phase else 0, rounds)
        self._chk(self.L.dagcon_set_site_reads(self.h, C.byref(o)))

    def site_reads(self) -> dict:
        """dagcon_fetch_site_reads (copies): aln_tgt (uint32), aln_src (uint64) per taken alignment; ent_begin (uint64, one
        more); ent_site (uint64, index into pileup_sites()' arrays) and ent_code (uint8, cls | ins << 3) per entry; hap
        (uint8 per alignment) and phase (int8 per site), None when phase was off."""
        sr = SiteReads()
        self._chk(self.L.dagcon_fetch_site_reads(self.h, C.byref(sr)))
        ps = PileupSites()
        self._chk(self.L.dagcon_fetch_pileup_sites(self.h, C.byref(ps)))
        n = int(sr.n_aln)
        n_site = int(ps.site_begin[int(ps.n_targets)])

        def arr(ptr, k, dt):
            return np.ctypeslib.as_array(ptr, shape=(k,)).copy() if k else np.zeros(0, dt)
        begin = np.ctypeslib.as_array(sr.ent_begin, shape=(n + 1,)).copy()
        ne = int(begin[n])
        return {"aln_tgt": arr(sr.aln_tgt, n, np.uint32), "aln_src": arr(sr.aln_src, n, np.uint64), "ent_begin": begin,
                "ent_site": arr(sr.ent_site, ne, np.uint64), "ent_code": arr(sr.ent_code, ne, np.uint8),
                "hap": arr(sr.hap, n, np.uint8) if sr.hap else None,
                "phase": arr(sr.phase, n_site, np.int8) if sr.phase else None}

    def set_site_alleles(self, on=True):
        """dagcon_set_site_alleles for every later upload made with set_pileup and set_site_reads on: the device groups and
        counts the alleles themselves at each site (site_alleles())."""
        self._chk(self.L.dagcon_set_site_alleles(self.h, 1 if on else 0))

    def site_alleles(self) -> dict:
        """dagcon_fetch_site_alleles (copies): al_begin (uint64, one per site of pileup_sites() and one more); key (uint64),
        count (uint32) and hap_count (uint16, [alleles, 3]: c1 c2 c0; None when phase was off) per allele; ent_allele
        (uint16, per entry of site_reads(): the index of its allele within its site's table)."""
        sa = SiteAlleles()
        self._chk(self.L.dagcon_fetch_site_alleles(self.h, C.byref(sa)))
        ns, ne = int(sa.n_sites), int(sa.n_ent)

        def arr(ptr, k, dt):
            return np.ctypeslib.as_array(ptr, shape=(k,)).copy() if k else np.zeros(0, dt)
        begin = np.ctypeslib.as_array(sa.al_begin, shape=(ns + 1,)).copy()
        n = int(begin[ns])
        return {"al_begin": begin, "key": arr(sa.key, n, np.uint64), "count": arr(sa.count, n, np.uint32),
                "hap_count": (arr(sa.hap_count, 3 * n, np.uint16).reshape(n, 3) if sa.hap_count else None),
                "ent_allele": arr(sa.ent_allele, ne, np.uint16)}

    def set_site_join(self, on=True):
        """dagcon_set_site_join for every later upload made with set_pileup, set_site_reads and set_site_alleles on: the
        device joins adjacent sites into runs and counts what the alignments show at all of a run's sites (joined_sites())."""
        self._chk(self.L.dagcon_set_site_join(self.h, 1 if on else 0))

    def joined_sites(self) -> dict:
        """dagcon_fetch_joined_sites (copies): run_begin (uint64, one per run and one more, into the sites of
        pileup_sites()); spanning, partial (uint32 per run); jal_begin (uint64, one per run and one more); key (uint64),
        count (uint32) and hap_count (uint16, [joined alleles, 3]: c1 c2 c0; None when phase was off) per joined allele;
        ent_joined (uint16, per entry of site_reads(): the index within its run's table, 0xFFFF for a partial member)."""
        js = JoinedSites()
        self._chk(self.L.dagcon_fetch_joined_sites(self.h, C.byref(js)))
        nr, ne = int(js.n_runs), int(js.n_ent)

        def arr(ptr, k, dt):
            return np.ctypeslib.as_array(ptr, shape=(k,)).copy() if k else np.zeros(0, dt)
        begin = np.ctypeslib.as_array(js.jal_begin, shape=(nr + 1,)).copy()
        n = int(begin[nr])
        return {"run_begin": np.ctypeslib.as_array(js.run_begin, shape=(nr + 1,)).copy(), "spanning": arr(js.spanning, nr, np.uint32),
                "partial": arr(js.partial, nr, np.uint32), "jal_begin": begin, "key": arr(js.key, n, np.uint64),
                "count": arr(js.count, n, np.uint32),
                "hap_count": (arr(js.hap_count, 3 * n, np.uint16).reshape(n, 3) if js.hap_count else None),
                "ent_joined": arr(js.ent_joined, ne, np.uint16)}

    def set_hap_consensus(self, min_sites=0, min_reads=0):
        """dagcon_set_hap_consensus for every later upload made with set_pileup and set_site_reads(True) on: the device
        tallies how well the two labels separate (hap_tally()) and upload_haps() derives a batch of two groups per split
        target.  0, 0: the defaults 2 and 3.  set_hap_consensus(None): off."""
        if min_sites is None:
            self._chk(self.L.dagcon_set_hap_consensus(self.h, None))
            return
        o = HapOpts(min_sites, min_reads)
        self._chk(self.L.dagcon_set_hap_consensus(self.h, C.byref(o)))

    def hap_tally(self) -> dict:
        """dagcon_fetch_hap_tally (copies): n1, n2, n0, n_sep, agree, disagree (uint32) and split (uint8) per target;
        site_counts (uint16, [sites, 4]: P1 M1 P2 M2 per site of pileup_sites())."""
        ht = HapTally()
        self._chk(self.L.dagcon_fetch_hap_tally(self.h, C.byref(ht)))
        ps = PileupSites()
        self._chk(self.L.dagcon_fetch_pileup_sites(self.h, C.byref(ps)))
        T = int(ht.n_targets)
        n_site = int(ps.site_begin[int(ps.n_targets)])
        out = {k: (np.ctypeslib.as_array(getattr(ht, k), shape=(T,)).copy() if T else np.zeros(0, np.uint32))
               for k in ("n1", "n2", "n0", "n_sep", "agree", "disagree")}
        out["split"] = np.ctypeslib.as_array(ht.split, shape=(T,)).copy() if T else np.zeros(0, np.uint8)
        out["site_counts"] = np.ctypeslib.as_array(ht.site_counts, shape=(n_site, 4)).copy() if n_site else np.zeros((0, 4), np.uint16)
        return out

    def upload_haps(self, swap=None):
        """dagcon_upload_haps: the batch of the groups, built from what the first batch left on the device; then run(),
        sync(), fetch() as after any upload.  swap (one byte per target of the first batch): dagcon_upload_haps_swapped,
        the two groups of a split target t with swap[t] != 0 change names."""
        if swap is None:
            self._chk(self.L.dagcon_upload_haps(self.h))
            return
        sw = np.ascontiguousarray(swap, dtype=np.uint8)
        self._chk(self.L.dagcon_upload_haps_swapped(self.h, sw.ctypes.data))

    def set_window_keep(self, lo, hi=None):
        """dagcon_set_window_keep for every later windows upload and every upload_haps() behind one: lo and hi per window
        of the first batch (copied); window_keep() then lists the kept part of every segment.  set_window_keep(None): off."""
        if lo is None:
            self._chk(self.L.dagcon_set_window_keep(self.h, None))
            return
        lo = np.ascontiguousarray(lo, dtype=np.uint32)
        hi = np.ascontiguousarray(hi, dtype=np.uint32)
        if lo.shape != hi.shape or lo.ndim != 1:
            raise ValueError("lo and hi are one array each, of one length")
        u32p = C.POINTER(C.c_uint32)
        o = WindowKeepOpts(len(lo), lo.ctypes.data_as(u32p), hi.ctypes.data_as(u32p))
        self._chk(self.L.dagcon_set_window_keep(self.h, C.byref(o)))

    def window_keep(self) -> dict:
        """dagcon_fetch_window_keep (copies): i0, i1, p_first, p_last (uint32), one per segment of the last results, in
        their order."""
        wk = WindowKeep()
        self._chk(self.L.dagcon_fetch_window_keep(self.h, C.byref(wk)))
        n = int(wk.n_segments)
        return {k: np.ctypeslib.as_array(getattr(wk, k), shape=(n,)).copy() if n else np.zeros(0, np.uint32)
                for k in ("i0", "i1", "p_first", "p_last")}

    def set_site_link(self, max_conflict_ppm=0, min_cell=0, min_partners=0, reach=0):
        """dagcon_set_site_link for every later upload made with set_pileup and set_site_reads(True) on: the device picks
        the sites that the same reads carry as other sites near them (site_link()) and the split, the tally and every
        label count take the other sites' entries as unsigned.  0 in a field: its default (100000, 3, 2, 256).
        set_site_link(None): off."""
        if max_conflict_ppm is None:
            self._chk(self.L.dagcon_set_site_link(self.h, None))
            return
        o = SiteLinkOpts(max_conflict_ppm, min_cell, min_partners, reach)
        self._chk(self.L.dagcon_set_site_link(self.h, C.byref(o)))

    def site_link(self) -> dict:
        """dagcon_fetch_site_link (copies): partners (uint16) and linked (uint8) per site of pileup_sites()."""
        sl = SiteLink()
        self._chk(self.L.dagcon_fetch_site_link(self.h, C.byref(sl)))
        n = int(sl.n_sites)
        return {"partners": np.ctypeslib.as_array(sl.partners, shape=(n,)).copy() if n else np.zeros(0, np.uint16),
                "linked": np.ctypeslib.as_array(sl.linked, shape=(n,)).copy() if n else np.zeros(0, np.uint8)}

    def hap_map(self) -> dict:
        """dagcon_fetch_hap_map (copies): src_target (uint32) and label (uint8) per target of the derived batch, aln_begin
        (uint64, one more) and aln_src (uint64, the caller's index of each of its alignments)."""
        hm = HapMap()
        self._chk(self.L.dagcon_fetch_hap_map(self.h, C.byref(hm)))
        T = int(hm.n_targets)
        begin = np.ctypeslib.as_array(hm.aln_begin, shape=(T + 1,)).copy()
        n = int(begin[T])
        return {"src_target": np.ctypeslib.as_array(hm.src_target, shape=(T,)).copy() if T else np.zeros(0, np.uint32),
                "label": np.ctypeslib.as_array(hm.label, shape=(T,)).copy() if T else np.zeros(0, np.uint8),
                "aln_begin": begin,
                "aln_src": np.ctypeslib.as_array(hm.aln_src, shape=(n,)).copy() if n else np.zeros(0, np.uint64)}

    def set_hap_calls(self, on=True):
        """dagcon_set_hap_calls (needs set_edits on): the batch upload_haps() derives from a record upload that ran with
        the edits reports its own edits (and their support, if the first batch had it) and pairs the two groups' edits
        (hap_calls())."""
        self._chk(self.L.dagcon_set_hap_calls(self.h, 1 if on else 0))

    def hap_calls(self) -> dict:
        """dagcon_fetch_hap_calls (copies): per edit of edits() its state (uint8: HC_NOCOVER, HC_HET, HC_CLASH, HC_HOM) and
        its mate (uint64 index into the same arrays, HC_NONE: none)."""
        hc = HapCalls()
        self._chk(self.L.dagcon_fetch_hap_calls(self.h, C.byref(hc)))
        n = int(hc.n)
        return {"state": np.ctypeslib.as_array(hc.state, shape=(n,)).copy() if n else np.zeros(0, np.uint8),
                "mate": np.ctypeslib.as_array(hc.mate, shape=(n,)).copy() if n else np.zeros(0, np.uint64)}

    def set_window_phase(self, min_links=0, max_conflict_ppm=0):
        """dagcon_set_window_phase for every later windows upload made with set_pileup and set_site_reads(True) on: the
        device joins the labels of neighbouring windows into blocks (window_phase()).  0, 0: the defaults 3 and 250000.
        set_window_phase(None): off."""
        if min_links is None:
            self._chk(self.L.dagcon_set_window_phase(self.h, None))
            return
        o = WindowPhaseOpts(min_links, max_conflict_ppm)
        self._chk(self.L.dagcon_set_window_phase(self.h, C.byref(o)))

    def window_phase(self) -> dict:
        """dagcon_fetch_window_phase (copies): same, diff, block (uint32) and flip (uint8) per window; hap (uint8, oriented,
        per alignment of site_reads()) and phase (int8, oriented, per site of pileup_sites())."""
        wp = WindowPhase()
        self._chk(self.L.dagcon_fetch_window_phase(self.h, C.byref(wp)))
        W, n, ns = int(wp.n_windows), int(wp.n_aln), int(wp.n_sites)

        def arr(ptr, k, dt):
            return np.ctypeslib.as_array(ptr, shape=(k,)).copy() if k else np.zeros(0, dt)
        return {"same": arr(wp.same, W, np.uint32), "diff": arr(wp.diff, W, np.uint32), "block": arr(wp.block, W, np.uint32),
                "flip": arr(wp.flip, W, np.uint8), "hap": arr(wp.hap, n, np.uint8), "phase": arr(wp.phase, ns, np.int8)}

    def edits(self) -> dict:
        """dagcon_fetch_edits (copies): seg_t0, seg_t1 (uint32, one per segment of the last results, in their order),
        edit_begin (uint64, one more), and per edit t_pos, t_len, c_len (uint32) and c_off (uint64, into seq_blob)."""
        e = Edits()
        self._chk(self.L.dagcon_fetch_edits(self.h, C.byref(e)))
        S, n = int(e.n_segments), int(e.n)

        def arr(ptr, k, dt):
            return np.ctypeslib.as_array(ptr, shape=(k,)).copy() if k else np.zeros(0, dt)
        return {"seg_t0": arr(e.seg_t0, S, np.uint32), "seg_t1": arr(e.seg_t1, S, np.uint32),
                "edit_begin": arr(e.edit_begin, S + 1, np.uint64), "t_pos": arr(e.t_pos, n, np.uint32),
                "t_len": arr(e.t_len, n, np.uint32), "c_off": arr(e.c_off, n, np.uint64), "c_len": arr(e.c_len, n, np.uint32)}

    def timings(self) -> dict:
        t = Timings()
        self._chk(self.L.dagcon_get_timings(self.h, C.byref(t)))
        return {k: getattr(t, k) for k, _ in Timings._fields_ if k != "reserved"}

    def normalize(self, alns, trim=0, raw=False):
        """alns = [(start, qstr, tstr)] -> [(start', qnorm, tnorm)] on the device:
        normalizeGaps then trimAln(trim); raw=True gives trimAln alone."""
        n = len(alns)
        starts = np.array([a[0] for a in alns], dtype=np.uint32)
        lens = np.array([len(a[1]) for a in alns], dtype=np.uint32)
        offs = np.zeros(n, dtype=np.uint64)
        if n:
            offs[1:] = np.cumsum(lens[:-1], dtype=np.uint64)
        q = np.frombuffer(b"".join(a[1] for a in alns) or b"\0", dtype=np.uint8)
        t = np.frombuffer(b"".join(a[2] for a in alns) or b"\0", dtype=np.uint8)
        out_off = 2 * offs
        total = int(2 * lens.sum()) + 1
        qout, tout = np.zeros(total, dtype=np.uint8), np.zeros(total, dtype=np.uint8)
        out_len, out_start = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32)
        self._chk(self.L.dagcon_normalize(
            self.h, n, starts.ctypes.data, offs.ctypes.data, lens.ctypes.data, q.ctypes.data,
            t.ctypes.data, int(lens.sum()), trim, FLAG_RAW_ALIGNMENTS if raw else 0, out_off.ctypes.data, qout.ctypes.data,
            tout.ctypes.data, out_len.ctypes.data, out_start.ctypes.data))
        res = []
        for a in range(n):
            o, m = int(out_off[a]), int(out_len[a])
            res.append((int(out_start[a]), qout[o:o + m].tobytes(), tout[o:o + m].tobytes()))
        return res

    def align(self, pairs):
        """pairs = [(qseq, tseq)] of unaligned sequences -> [(qaln, taln)] (the -a stage, SimpleAligner.cpp:25-63)."""
        n = len(pairs)
        self._align_n = n
        if n == 0:
            return []
        ql = np.array([len(q) for q, _ in pairs], dtype=np.uint32)
        tl = np.array([len(t) for _, t in pairs], dtype=np.uint32)
        qo, to, oo = np.zeros(n, np.uint64), np.zeros(n, np.uint64), np.zeros(n, np.uint64)
        qo[1:] = np.cumsum(ql[:-1], dtype=np.uint64)
        to[1:] = np.cumsum(tl[:-1], dtype=np.uint64)
        oo[1:] = np.cumsum((ql[:-1].astype(np.uint64) + tl[:-1]), dtype=np.uint64)
        qb = np.frombuffer(b"".join(q for q, _ in pairs) or b"\0", dtype=np.uint8)
        tb = np.frombuffer(b"".join(t for _, t in pairs) or b"\0", dtype=np.uint8)
        total = int(ql.sum()) + int(tl.sum()) + 1
        qa, ta = np.zeros(total, np.uint8), np.zeros(total, np.uint8)
        ln = np.zeros(n, np.uint32)
        self._chk(self.L.dagcon_align(self.h, n, qo.ctypes.data, ql.ctypes.data, to.ctypes.data, tl.ctypes.data,
                                      qb.ctypes.data, int(ql.sum()), tb.ctypes.data, int(tl.sum()), oo.ctypes.data,
                                      qa.ctypes.data, ta.ctypes.data, ln.ctypes.data))
        return [(qa[int(oo[a]):int(oo[a]) + int(ln[a])].tobytes(), ta[int(oo[a]):int(oo[a]) + int(ln[a])].tobytes())
                for a in range(n)]

    def align_panels(self, pairs, panels):
        """pairs = [(qseq, tseq)] (B interval, A interval), panels[a] = [(A bases, B bases)] per trace-point panel
        -> ([(qaln, taln)], [[distance per panel]]) (dagcon_align_panels; an overlap with a panel larger than
        DAGCON_PANEL_MAX_SIDE comes back as (b"", b"") with distances -1, and counts in align_dropped())."""
        n = len(pairs)
        if n == 0:
            return [], []
        ql = np.array([len(q) for q, _ in pairs], dtype=np.uint32)
        tl = np.array([len(t) for _, t in pairs], dtype=np.uint32)
        qo, to, oo = np.zeros(n, np.uint64), np.zeros(n, np.uint64), np.zeros(n, np.uint64)
        qo[1:] = np.cumsum(ql[:-1], dtype=np.uint64)
        to[1:] = np.cumsum(tl[:-1], dtype=np.uint64)
        oo[1:] = np.cumsum((ql[:-1].astype(np.uint64) + tl[:-1]), dtype=np.uint64)
        pb = np.zeros(n + 1, np.uint64)
        pb[1:] = np.cumsum([len(p) for p in panels], dtype=np.uint64)
        np_ = int(pb[-1])
        ptl = np.array([x for p in panels for x, _ in p] or [0], dtype=np.uint32)
        pql = np.array([y for p in panels for _, y in p] or [0], dtype=np.uint32)
        qb = np.frombuffer(b"".join(q for q, _ in pairs) or b"\0", dtype=np.uint8)
        tb = np.frombuffer(b"".join(t for _, t in pairs) or b"\0", dtype=np.uint8)
        total = int(ql.sum()) + int(tl.sum()) + 1
        qa, ta = np.zeros(total, np.uint8), np.zeros(total, np.uint8)
        ln = np.zeros(n, np.uint32)
        dist = np.zeros(max(np_, 1), np.int32)
        self._chk(self.L.dagcon_align_panels(self.h, n, qo.ctypes.data, ql.ctypes.data, to.ctypes.data, tl.ctypes.data,
                                             qb.ctypes.data, int(ql.sum()), tb.ctypes.data, int(tl.sum()), pb.ctypes.data,
                                             ptl.ctypes.data, pql.ctypes.data, oo.ctypes.data, qa.ctypes.data,
                                             ta.ctypes.data, ln.ctypes.data, dist.ctypes.data))
        alns = [(qa[int(oo[a]):int(oo[a]) + int(ln[a])].tobytes(), ta[int(oo[a]):int(oo[a]) + int(ln[a])].tobytes())
                for a in range(n)]
        return alns, [dist[int(pb[a]):int(pb[a + 1])].tolist() for a in range(n)]

    def align_ends(self):
        """[(q_begin, q_end, t_begin, t_end)] of the last align / consensus_pre (dagcon_align_ends): the aligned strings
        cover q[q_begin:q_end] and t[t_begin:t_end].  Local with FLAG_LOCAL_ALIGN, else the whole of both."""
        n = self._align_n
        e = np.zeros((4, max(n, 1)), np.uint32)
        self._chk(self.L.dagcon_align_ends(self.h, n, e[0].ctypes.data, e[1].ctypes.data, e[2].ctypes.data,
                                           e[3].ctypes.data))
        return [tuple(int(x) for x in e[:, a]) for a in range(n)]

    def place(self, seqs, pairs, k=12, max_occ=4):
        """seqs = [bytes], pairs = [(q, t)] indices into seqs -> dict of numpy arrays over the pairs (dagcon_place):
        votes_fwd, votes_rev (uint32), strand (bytes: b'+', b'-' or b'.' per pair), t0, t1 (uint32)."""
        n = len(pairs)
        ln = np.array([len(s) for s in seqs] or [0], dtype=np.uint32)
        off = np.zeros(max(len(seqs), 1), np.uint64)
        if len(seqs) > 1:
            off[1:] = np.cumsum(ln[:-1], dtype=np.uint64)
        blob = np.frombuffer(b"".join(seqs) or b"\0", dtype=np.uint8)
        pr = np.array(pairs, dtype=np.uint32).reshape(-1, 2) if n else np.zeros((0, 2), np.uint32)
        pq, pt = np.ascontiguousarray(pr[:, 0]), np.ascontiguousarray(pr[:, 1])
        out = {name: np.zeros(max(n, 1), np.uint32) for name in ("votes_fwd", "votes_rev", "t0", "t1")}
        strand = np.zeros(max(n, 1), np.uint8)
        self._chk(self.L.dagcon_place(self.h, off.ctypes.data, ln.ctypes.data, blob.ctypes.data,
                                      sum(len(s) for s in seqs), n, pq.ctypes.data, pt.ctypes.data, k, max_occ,
                                      out["votes_fwd"].ctypes.data, out["votes_rev"].ctypes.data, strand.ctypes.data,
                                      out["t0"].ctypes.data, out["t1"].ctypes.data))
        res = {name: a[:n] for name, a in out.items()}
        res["strand"] = strand[:n].tobytes()
        return res

    def align_dropped(self):
        """Pairs the last align / align_panels / consensus_pre left unaligned (dagcon_align_dropped)."""
        return int(self.L.dagcon_align_dropped(self.h))

    def consensus_pre(self, targets, strict=True):
        """targets = [(tlen, [(tstart, strand, qseq, tseq)])]: .pre records per target (Alignment.cpp:82-112)
        -> per target [(range0, range1, seq_bytes)] (dagcon_consensus_pre: main.cpp:117-145 with -a)."""
        recs = [r for _, rs in targets for r in rs]
        n = len(recs)
        self._align_n = n
        tlen = np.array([t for t, _ in targets], dtype=np.uint32)
        begin = np.zeros(len(targets) + 1, np.uint64)
        begin[1:] = np.cumsum([len(rs) for _, rs in targets], dtype=np.uint64)
        ts = np.array([r[0] for r in recs] or [0], dtype=np.uint32)
        strand = np.frombuffer(b"".join(r[1] for r in recs) or b"+", dtype=np.uint8)
        ql = np.array([len(r[2]) for r in recs] or [0], dtype=np.uint32)
        tl = np.array([len(r[3]) for r in recs] or [0], dtype=np.uint32)
        qo, to = np.zeros(max(n, 1), np.uint64), np.zeros(max(n, 1), np.uint64)
        qo[1:] = np.cumsum(ql[:-1], dtype=np.uint64)
        to[1:] = np.cumsum(tl[:-1], dtype=np.uint64)
        qb = np.frombuffer(b"".join(r[2] for r in recs) or b"\0", dtype=np.uint8)
        tb = np.frombuffer(b"".join(r[3] for r in recs) or b"\0", dtype=np.uint8)
        pb = PreBatch(len(targets), tlen.ctypes.data, begin.ctypes.data, ts.ctypes.data, strand.ctypes.data,
                      qo.ctypes.data, ql.ctypes.data, to.ctypes.data, tl.ctypes.data, qb.ctypes.data,
                      int(ql.sum()) if n else 0, tb.ctypes.data, int(tl.sum()) if n else 0)
        r = Results()
        self.L.dagcon_consensus_pre.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        self._chk(self.L.dagcon_consensus_pre(self.h, C.byref(pb), C.byref(r)))
        out = self._keep_segs(r)
        self._status(r, strict)
        return out

    def debug_counters(self):
        a = (C.c_ulonglong * 16)()
        self.L.dagcon_debug_counters.argtypes = [C.c_void_p, C.c_void_p]
        self._chk(self.L.dagcon_debug_counters(self.h, a))
        return list(a)

    def debug_graph(self, target=0):
        """Per vertex (device ids, backbone-position order):
        dict(base, weight, coverage, deleted, backbone, bbpos, out=[(dst,count)], inn=[src])."""
        d = GraphDump()
        self._chk(self.L.dagcon_debug_graph(self.h, target, C.byref(d)))
        out = []
        for v in range(d.n_nodes):
            oe = [(d.out_dst[i], d.out_count[i]) for i in range(d.out_begin[v], d.out_begin[v + 1])]
            ie = [d.in_src[i] for i in range(d.in_begin[v], d.in_begin[v + 1])]
            out.append(dict(base=chr(d.base[v]), weight=d.weight[v], coverage=d.coverage[v],
                            deleted=bool(d.deleted[v]), backbone=bool(d.backbone[v]), bbpos=d.bbpos[v],
                            out=oe, inn=ie))
        return out


def _results_to_py(r: Results):
    T = r.n_targets
    blob = C.string_at(r.seq_blob, r.seq_bytes) if r.seq_bytes else b""
    out = []
    for t in range(T):
        segs = []
        for s in range(r.seg_begin[t], r.seg_begin[t + 1]):
            o, n = r.seq_off[s], r.seq_len[s]
            segs.append((r.range0[s], r.range1[s], blob[o:o + n]))
        out.append(segs)
    return out
