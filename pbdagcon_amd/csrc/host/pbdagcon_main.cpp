// pbdagcon_main.cpp -- `pbdagcon`-compatible command line on top of the C ABI.
//
// Replaces the Reader -> N x Consensus -> Writer thread pipeline of the reference
// (src/cpp/main.cpp:37-176, 227-288) with: parse the BLASR -m 5 stream, group
// consecutive records by target id (BlasrM5AlnProvider.cpp:34-55), hand batches of
// independent targets to dagcon_consensus() (include/dagcon.h), print FASTA records in
// input order (main.cpp:141-143).  Same flags and defaults as main.cpp:178-225.
//
// The parser thread fills one batch while a second thread has the previous one on the GPU
// (context creation included, so HIP start-up hides behind the first batch's parsing).
//
// Differences that are deliberate and documented in DESIGN.md:
//   * output order is input order (the reference's is nondeterministic for -j >= 2, Q3);
//   * -j is the number of host threads that index the text and copy the strings (the consensus
//     itself is the GPU's), -j 1 does not deadlock (Q2);
//   * -a (.pre input, every record re-aligned first: main.cpp:127-128, 243-246) runs this build's own
//     banded aligner on the GPU (dagcon_align): blasr_libcpp is absent, the stage is pinned to the
//     reference by its one known-answer test only (test/cpp/SimpleAlignerTest.cpp:8-21); global by
//     default, local ends with --local (DAGCON_FLAG_LOCAL_ALIGN, the reference's SDPAlign(..., Local));
//   * --sam, --bam, --paf --reads and --paf --cs, all with --ref: alignment records (a position, a CIGAR or cs:Z: text and the
//     ungapped read, or no read at all) against a FASTA of the targets; what each format gives is in sam.h, bam.h and paf.h, the one
//     record they all become and the per-kind description in intake.h.  The gapped strings are made on the GPU, never on the host;
//   * --sam --md and --bam --md need no --ref: the targets' names and lengths come from the header, every record's MD:Z: text goes
//     to the GPU, which rebuilds the target bases from CIGAR, SEQ and that text (include/dagcon.h, dagcon_md_tags);
//   * blank lines are skipped (the reference duplicates the previous record, Q9);
//   * a missing input file is an error on stderr, exit 1 (the reference is silent, Q11).
#include <algorithm>
#include <cerrno>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <condition_variable>
#include <mutex>
#include <string>
#include <chrono>
#include <thread>
#include <unordered_set>
#include <utility>
#include <vector>

#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include "../../../include/dagcon.h"
#include "bam.h"
#include "fastq.h"
#include "paf.h"
#include "sam.h"
#include "windows.h"
#include "vcf.h"
#include "pileup.h"
#include "site_reads.h"
#include "alleles.h"
#include "joined.h"
#include "hap.h"
#include "hap_vcf.h"

namespace {

enum Mode { MODE_M5, MODE_PRE, MODE_RECORDS };             // BLASR -m 5 text; .pre text (-a); alignment records of o.kind

struct Opts {
    unsigned threads = 4, min_cov = 6, min_len = 500, trim = 50;
    Mode mode = MODE_M5;                // what the input is, decided once by parse_args
    DgRecordKind kind = DG_REC_PLAIN;   // MODE_RECORDS: --sam, --bam, --paf, --paf --cs, --sam --md or --bam --md (intake.h)
    bool verbose = false, dump = false, local = false;   // local: --local (with -a), the first alignment of every record has local ends
    std::string ref, reads;            // --ref FASTA (MODE_RECORDS); --reads FASTA / FASTQ (with --paf)
    unsigned window = 0, overlap = 1000;   // --window W [--overlap O] (MODE_RECORDS): targets cut into windows (windows.h)
    bool overlap_set = false;
    DgPick pick;                       // --max-error F, --max-depth N (MODE_RECORDS): the records are picked on the device
    std::string edits;                 // --edits FILE (MODE_RECORDS): where every record differs from its target
    std::string vcf;                   // --vcf FILE (MODE_RECORDS, whole targets): the edits as VCF with the reads behind each
    bool want_edits() const { return !edits.empty() || !vcf.empty() || !hap.vcf.empty(); }
    bool want_edit_support() const { return !vcf.empty() || !hap.vcf.empty(); }   // (--hap-vcf FILE: the edits with their support, for both runs)
    DgPileOpts pile;                   // --pileup FILE, --sites FILE [--site-min-frac F] [--site-min-count N] (every mode): what the alignments show per position
    std::string hap_contigs, hap_windows;   // --hap-contigs FILE, --hap-windows FILE (with --window --phase-windows): phased contigs across windows (hap_contigs.h)
    bool want_hc() const { return !hap_contigs.empty() || !hap_windows.empty(); }
    DgWinPhaseOpts wp;                 // --phase-windows [--phase-min-links N] [--phase-max-conflict F]: --site-reads / --haplotag with --window, the windows' labels joined (windows.h)
    DgSiteReadOpts sr;                 // --site-reads FILE, --haplotag FILE (whole targets, not -a): which read shows which allele at the sites; a two-way split
    DgLinkOpts link;                   // --link-sites [--link-*], --linked-sites FILE (where the split goes): only the sites the same reads carry sign the split
    DgHapOpts hap;                     // --hap-consensus FILE, --hap-sites FILE (where --haplotag goes): a consensus per group of the split, the split's tally; --hap-vcf FILE (records): the groups' edits paired
    DgAlleleOpts al;                   // --site-alleles FILE, --site-vcf FILE (where --site-reads goes): the alleles themselves at the sites, counted
    DgJoinedOpts jn;                   // --joined-alleles FILE, --joined-vcf FILE (where --site-alleles / --site-vcf go): adjacent sites joined into one record
    bool want_al() const { return al.on() || jn.on(); }               // (the joined sites need the alleles, whether or not their files are asked for)
    bool want_sr() const { return sr.on() || hap.on() || want_al(); }   // (the tally and the alleles need the site reads, whether or not their files are asked for)
    bool want_phase() const { return sr.phase() || hap.on(); }        // the split: --haplotag, --hap-consensus or --hap-sites
    bool want_pile() const { return pile.on() || want_sr(); } // (the site reads need the pile-up, whether or not its files are asked for)
    bool fastq = false;                // --fastq: FASTQ records, qualities from the per-base support (fastq.h)
    std::vector<int> devices{0};       // --devices: one consensus worker (thread + context) per GPU
    int pinned = -1;                   // --pinned 0|1: page-locked blobs (-1: when the input is several batches long)
    unsigned contexts = 0;             // --contexts N: consensus workers per GPU (0: two when the input is several batches long)
    unsigned polish = 0;               // --polish N (with -a): N more rounds with the consensus as the new backbone
    size_t batch_targets = 512;        // parsing and the GPU still overlap on mid-size inputs; 256 left the GPU a third less efficient (4,000 targets: 0.79 -> 0.67 s)
    size_t batch_bytes = 512ull << 20;  // (of strings: 80 targets of 50 kb x 60x fill the chip; what a context holds, and has to allocate on its first batch, grows with it)
    size_t slab_bytes = 0;             // test hook: text indexed per round (0 = automatic)
    std::string input;
};


void usage(FILE *f) {
    fprintf(f,
            "USAGE: pbdagcon [-j <int>] [-c <uint>] [-m <uint>] [-t <uint>] [-a [--local]] [--sam|--bam --ref <fasta> | --sam|--bam --md | --paf --ref <fasta> --reads <fasta|fastq> | --paf --cs --ref <fasta> [--window W [--overlap O]] [--max-error F] [--max-depth N] [--edits FILE] [--vcf FILE]] [--pileup FILE] [--sites FILE [--site-min-frac F] [--site-min-count N]] [--site-reads FILE] [--haplotag FILE] [--hap-consensus FILE [--hap-min-sites N] [--hap-min-reads N]] [--hap-sites FILE] [--fastq] [--site-alleles FILE] [--site-vcf FILE] [--joined-alleles FILE] [--joined-vcf FILE] [--hap-vcf FILE] [--window W --phase-windows --hap-contigs FILE [--hap-windows FILE]] [--link-sites [--link-max-conflict F] [--link-min-cell N] [--link-min-partners N] [--link-reach N]] [--linked-sites FILE] [-v] <input>\n"
            "  PBDAGCON is a tool that implements DAGCon (Directed Acyclic Graph Consensus); this build\n"
            "  runs the consensus on an MI355X through libdagcon_hip.so.\n"
            "  -j, --threads       host threads for parsing (default 4); the consensus runs on the GPU\n"
            "  -c, --min-coverage  minimum alignments per target, also the minimum node weight (default 6)\n"
            "  -m, --min-length    minimum alignment / consensus length (default 500)\n"
            "  -t, --trim          trim alignments on either side (default 50)\n"
            "  -a, --align         input is .pre (qid tid strand tlen tstart tend qseq tseq): align the sequences first\n"
            "                      (this build's own banded aligner on the GPU, global unless --local; the reference's blasr\n"
            "                      SDPAlign(Local) + GuidedAlign is not in its tree: parity unpinned beyond its one SimpleAligner\n"
            "                      known-answer test)\n"
            "  --local             with -a: align local ends, so read ends that do not align stay out of the graph (the record\n"
            "                      starts at tstart + the first aligned target base); --polish rounds stay global\n"
            "  --sam               input is SAM text, records of one RNAME consecutive (a coordinate-sorted SAM is): FLAG, RNAME,\n"
            "                      POS, CIGAR and SEQ are used, the target's bases come from --ref; records with FLAG 0x4 or\n"
            "                      0x100, or RNAME, CIGAR or SEQ '*', are skipped (counted with -v).  The gapped strings are made\n"
            "                      on the GPU; the output is that of the .m5 input with the same alignments.  Not with -a,\n"
            "                      --local or --polish.  Without a FASTA: --md\n"
            "  --bam               input is BAM: everything --sam does, from the same records in a BAM file (BGZF inflated on the\n"
            "                      -j threads by this build's own decoder, CRC32 and ISIZE of every member checked).  refID, pos,\n"
            "                      flag, read_name, the CIGAR (from the CG tag when it has more than 65,535 ops) and seq are used;\n"
            "                      records with FLAG 0x4 or 0x100, refID < 0, no CIGAR or no SEQ are skipped (counted with -v);\n"
            "                      errors name the record's ordinal in the file.  The CIGAR ops and the 4-bit bases go to the GPU\n"
            "                      as they lie in the file.  Indexes, CRAM and QUAL are not read.  Parity unpinned: tested on\n"
            "                      files from this build's own BAM writer only\n"
            "  --paf               input is PAF with cg:Z: tags (minimap2 -c): everything --sam does, from qname qlen qs qe strand\n"
            "                      tname tlen ts te and the cg tag; the read bases come from --reads, the target's from --ref.\n"
            "                      A line's slice [qs, qe) of its read goes to the GPU as the reads file has it, and the GPU\n"
            "                      reads a '-' line's bases backwards and complemented (A<->T, C<->G, lower case too: this\n"
            "                      build's own rule, parity unpinned).  Lines are grouped by target: targets in --ref order,\n"
            "                      a target's lines in file order (with --window: ascending in ts).  tp:A:S lines are skipped\n"
            "                      (counted with -v); lines without cg:Z: are skipped and their count is printed.  A line\n"
            "                      whose lengths disagree with the files, or that names an unknown sequence, is an error.\n"
            "                      Not with --sam, --bam, -a, --local or --polish.  MD:Z:, QUAL and gzip are not read\n"
            "  --cs                with --paf, instead of --reads: the lines carry cs:Z: tags (minimap2 --cs, short or long form,\n"
            "                      with or without -c).  A cs:Z: tag and the target are the whole alignment: there is no reads\n"
            "                      file, the query name is not looked up, and a '-' line needs nothing done to it.  The tag's\n"
            "                      text goes to the GPU as it lies in the file and is decoded there (:n copies the target's\n"
            "                      bytes, =SEQ *tq +SEQ give upper-cased read bases, -SEQ none; ~ is not taken: this build's own\n"
            "                      rule, parity unpinned).  A line whose text does not give qe - qs read bases and te - ts target\n"
            "                      bases, or breaks the grammar, takes its target (with --window: the windows it touches) out\n"
            "                      with a warning.  Lines without cs:Z: are skipped and their count is printed.  Everything\n"
            "                      else is as with --paf --reads.  Not with --reads, --sam, --bam, -a, --local or --polish\n"
            "  --md                with --sam or --bam, instead of --ref: no FASTA is needed.  Every record carries an MD:Z: tag\n"
            "                      (BWA always writes it; minimap2 --MD and samtools calmd add it), which with CIGAR and SEQ\n"
            "                      spells every target base the record touches.  The tag's text goes to the GPU as it lies in\n"
            "                      the file, and the GPU rebuilds the targets: a base a letter of any record spells (a mismatch,\n"
            "                      a deleted base) is that letter, otherwise the read base of a record that matches there, N\n"
            "                      where no record reaches.  Target names and lengths come from the @SQ lines (--bam: the file's\n"
            "                      reference list); a record whose RNAME has none is an error.  The text must match\n"
            "                      [0-9]+(([A-Za-z]|^[A-Za-z]+)[0-9]+)* with numbers of at most 9 digits below 2^28 and cover\n"
            "                      exactly the target bases of the CIGAR, else the record takes its target (with --window: the\n"
            "                      windows it touches) out with a warning; so do all records of a target whose tags disagree\n"
            "                      about a base.  Records without the tag are skipped and their count is printed.  --window,\n"
            "                      --fastq, --edits (REF is the rebuilt target), --max-error and --max-depth work as with --ref.\n"
            "                      This build's own rule, parity unpinned.  Not with --ref, --paf, -a, --local or --polish\n"
            "  --reads FILE        with --paf (required): the reads, FASTA (multi-line) or four-line FASTQ by the first byte,\n"
            "                      named by the first word of the header; a name that occurs twice is an error\n"
            "  --ref FASTA         with --sam, --bam or --paf (required): the target sequences, by the name up to the first blank; an @SQ line\n"
            "                      whose LN differs from the sequence of its SN is an error\n"
            "  --window W          with --sam, --bam or --paf: targets of any length and depth.  Every target is cut into windows with cores of W\n"
            "                      bases, each run with --overlap more bases on either side; the records are cut to the windows\n"
            "                      on the GPU and the windows' consensus is joined at target coordinates.  Records of one RNAME\n"
            "                      must then be ascending in POS (a coordinate-sorted SAM).  In this mode only, a record is named\n"
            "                      >RNAME/t0_t1 with t0, t1 TARGET coordinates (0-based start, end) of its first and last base,\n"
            "                      not indexes into the consensus string; a break in the consensus starts a new record\n"
            "  --overlap O         with --window: bases a window is widened by on either side (default 1000); at least\n"
            "                      --trim + 64, so that trimming at a window's ends does not thin the coverage inside its core\n"
            "  --phase-windows     with --window and --site-reads FILE and / or --haplotag FILE: the two-way read split across\n"
            "                      the windows.  Every window is split on its own; a read that crosses a window boundary has a\n"
            "                      piece, and a label, in both windows.  A window is linked to the one in front when at least\n"
            "                      --phase-min-links N (default 3) such reads agree on how the two windows' labels correspond\n"
            "                      and at most the fraction --phase-max-conflict F (default 0.25; decimal text with at most six\n"
            "                      places) of them disagree; linked windows form a block with one naming of the labels, found\n"
            "                      on the GPU.  --site-reads FILE then has the lines of the sites inside the windows' cores,\n"
            "                      POS in target coordinates; --haplotag FILE has one line per record with a piece the graph\n"
            "                      took, RNAME QNAME HAP SITES PS: HAP by the vote of the record's pieces in the block that holds\n"
            "                      most of them, PS 1 + the first core position of that block (. when no piece has a label).\n"
            "                      The consensus on stdout is unchanged.  This build's own rule, parity unpinned\n"
            "  --max-error F       with --sam, --bam or --paf: leave out the records whose read disagrees with the target in more\n"
            "                      than the fraction F of the alignment's columns (mismatches + inserted + deleted bases; = and X\n"
            "                      ops are not trusted, the bases are compared, case ignored).  F is decimal text in [0, 1] with\n"
            "                      at most six places, e.g. 0.15.  Counted on the GPU from the records as they lie there; this\n"
            "                      build's own rule, parity unpinned\n"
            "  --max-depth N       with --sam, --bam or --paf: of the records --max-error leaves, at most N per target (with --window:\n"
            "                      per window) go into the graph, those with the most matching columns, in their own order; 1..4094.\n"
            "                      -c counts what is left.  With it a target or window of any depth can be run.  Both flags end\n"
            "                      with one line on stderr that counts the records each left out\n"
            "  --edits FILE        with --sam, --bam or --paf, with or without --window: FILE lists where every record\n"
            "                      differs from its target.  A line '#piece RNAME t0 t1' per record, in output order, with the\n"
            "                      target span [t0, t1) the record covers, then one line per edit: RNAME, begin, end (0-based,\n"
            "                      half-open target coordinates), REF, ALT, tab-separated, '-' for an empty side.  The edits\n"
            "                      applied to ref[t0:t1] give the record's sequence.  The list comes from the GPU, read off\n"
            "                      the best path itself, nothing is aligned again; stdout does not change.  This build's own\n"
            "                      rule, parity unpinned\n"
            "  --vcf FILE          with --sam, --bam or --paf (--ref or --md; not with --window): FILE lists the edits of --edits\n"
            "                      as VCFv4.2, one line per edit in output order: RNAME POS . REF ALT . . DP=span;AD=ref,alt;\n"
            "                      WIN=first-last.  DP counts the alignments that span the edit's window, AD those among them that\n"
            "                      carry the target's and the consensus' allele there, WIN is the window (every place the same\n"
            "                      change could be written in a repeat).  A pure insertion or deletion is anchored on the base in\n"
            "                      front of it (at position 1: behind it).  Counted on the GPU from the alignments as the graph\n"
            "                      took them; stdout and --edits do not change.  This build's own rule, parity unpinned\n"
            "  --pileup FILE       every kind of input, with or without --window (not with --polish): FILE lists, for every target\n"
            "                      position that an alignment covers, what the alignments the graph was built from show there,\n"
            "                      one line per position in output order: RNAME POS REF DEPTH A C G T N DEL INS, tab-separated.\n"
            "                      POS is 1-based; REF is the target's base with --sam, --bam and --paf and '.' otherwise;\n"
            "                      DEPTH = A + C + G + T + N + DEL; INS counts the alignments with inserted bases behind the\n"
            "                      position.  With --window a position's line comes from the window whose core holds it.\n"
            "                      Counted on the GPU; stdout does not change.  This build's own rule, parity unpinned\n"
            "  --sites FILE        the same lines, only for the positions where a second allele has support: with m the\n"
            "                      second largest of A C G T N DEL, or min(INS, DEPTH - INS) if that is more, a position is\n"
            "                      listed when m >= N and m >= F x DEPTH.  --site-min-frac F (default 0.2, at most six decimal\n"
            "                      places) and --site-min-count N (default 2) are this build's own choice.  Goes with --pileup\n"
            "  --site-reads FILE   every kind of input (not with --window, -a, --polish): FILE lists which read shows which allele at\n"
            "                      each position --sites would list (the same thresholds, --site-min-frac and --site-min-count, with\n"
            "                      or without --sites), one line per read and site: RNAME POS QNAME ALLELE INS, tab-separated, a\n"
            "                      target's sites ascending, a site's reads in the order of their records.  ALLELE is one of\n"
            "                      A C G T N *, * for a deleted base; INS is 1 when the read has inserted bases behind the position\n"
            "                      (which bases is not compared).  Only the alignments the graph was built from are listed.\n"
            "                      Listed on the GPU; stdout does not change.  This build's own rule, parity unpinned\n"
            "  --haplotag FILE     the same inputs: FILE has one line per alignment the graph was built from, RNAME QNAME HAP\n"
            "                      SITES.  The reads of a target are split in two groups that agree site after site: HAP is 1 or\n"
            "                      2, or 0 where a read has no informative site, ties, or lies more than 8 read overlaps from the\n"
            "                      read the split starts at; SITES is the number of the read's informative sites.  A heterozygous\n"
            "                      site or a collapsed repeat copy splits the reads the same way at every site, a systematic error\n"
            "                      does not.  The names 1 and 2 hold inside one target only.  This build's own rule, parity unpinned\n"
            "  --fastq             write FASTQ (@id/r0_r1, sequence, +, qualities) instead of FASTA; the same records in the\n"
            "                      same order.  The quality of a base is this build's own definition: a Laplace-smoothed\n"
            "                      fraction of the reads at its position that do not pass through its consensus vertex,\n"
            "                      with w = the vertex's weight, c = max(its backbone position's coverage, w), x = c - w + 1:\n"
            "                      Q = floor(10 log10((c + 2) / x)), in exact integer arithmetic, printed as 33 + Q\n"
            "                      (with --polish: the support of the last round)\n"
            "  --hap-consensus FILE  where --haplotag goes: a target whose reads split into two groups that separate at N or more\n"
            "                      sites (--hap-min-sites, default 2), each group with N or more reads (--hap-min-reads, default 3)\n"
            "                      and deep enough for -c, gets a consensus per group from a second run on the GPU, on the reads\n"
            "                      that are still there: a group is its labelled reads and the target's unlabelled ones.  FILE gets\n"
            "                      one FASTA record per segment, >RNAME/hap1/r0_r1 and >RNAME/hap2/r0_r1; the thresholds of the sites\n"
            "                      are --site-min-frac and --site-min-count.  stdout does not change.  This build's own rule, parity unpinned\n"
            "  --hap-sites FILE    the same inputs: one line per target, #target RNAME N1 N2 N0 SEP AGREE DISAGREE SPLIT (reads of label\n"
            "                      1, 2 and none, separating sites, entries that agree and disagree with the sites' phase, 1 when the\n"
            "                      target is split), and behind it one line per site with a phase: RNAME POS PHASE P1 M1 P2 M2, how many\n"
            "                      reads of label 1 and 2 show the site's first (P) and second (M) allele; POS is 1-based, as in\n"
            "                      --sites.  Counted on the GPU.  This build's own rule, parity unpinned\n"
            "  --site-alleles FILE where --site-reads goes: FILE lists the alleles themselves at each position --sites would list (the\n"
            "                      same thresholds), one line per allele: RNAME POS REF DEPTH ALLELE COUNT H1 H2 H0, tab-separated,\n"
            "                      a target's sites ascending, a site's alleles by COUNT descending.  ALLELE is what a read has\n"
            "                      between this target base and the next: its bases, - for none (a deleted base), so a\n"
            "                      substitution reads as the new base and an insertion as the kept base and the inserted ones; a\n"
            "                      trailing + says more than 20 bases (alleles that agree in the first 20 count as one).  H1 H2 H0\n"
            "                      are the COUNT reads by their group of the split, . unless --haplotag, --hap-consensus,\n"
            "                      --hap-sites or --hap-vcf is given.  Counted on the GPU; stdout does not change.  This build's own rule; the\n"
            "                      reference has no such output\n"
            "  --site-vcf FILE     with --sam, --bam or --paf: the same tables as VCFv4.2, one record per site that has an ALT:\n"
            "                      RNAME POS . REF ALT . . DP=depth;AD=ref,alt1,..  (and AD1=..;AD2=.. per group with the split on).\n"
            "                      ALT is every allele that is not the REF base, has no + and has COUNT >= --site-min-count; a\n"
            "                      deleted base takes the target base in front as anchor for the whole record (the base behind at\n"
            "                      position 1; a target of one base has no records).  Adjacent sites are NOT joined: a deletion\n"
            "                      of three bases is three records.  No genotype is called\n"
            "  --joined-alleles FILE where --site-alleles goes: adjacent positions that --sites would list are joined into runs (of\n"
            "                      at most 16; never across targets), and FILE lists what the reads that cover a whole run show\n"
            "                      over all of it, one line per joined allele: RNAME POS END REF SPAN PARTIAL ALLELE COUNT H1 H2 H0,\n"
            "                      tab-separated, POS and END 1-based inclusive, REF the target's bases there (. without them).\n"
            "                      SPAN reads cover every position of the run, PARTIAL only some; ALLELE is the alleles of\n"
            "                      --site-alleles one after the other, - for none (the whole run deleted), * when it cannot be\n"
            "                      spelled (a + allele, or one past the 15th of its position's table).  Counted on the GPU;\n"
            "                      stdout does not change.  This build's own rule; the reference has no such output\n"
            "  --joined-vcf FILE   with --sam, --bam or --paf: the same tables as VCFv4.2, one record per run that has an ALT:\n"
            "                      RNAME POS . REF ALT . . DP=span;PART=partial;AD=ref,alt1,..  (and AD1=..;AD2=.. with the split on).\n"
            "                      A deletion of three bases is one record, and two neighbouring substitutions carried by the\n"
            "                      same reads are one ALT.  ALT is every joined allele that is not *, differs from REF and has\n"
            "                      COUNT >= --site-min-count; an empty one takes the base in front as anchor (the base behind the\n"
            "                      run at position 1; a run that covers its whole target has no record).  Shared leading and\n"
            "                      trailing bases of REF and ALT are NOT trimmed.  No genotype is called\n"
            "  -v, --verbose       per-target progress on stderr\n"
            "  --hap-vcf FILE      with --sam, --bam or --paf, where --hap-consensus goes: diploid calls from the two groups' consensus,\n"
            "                      VCFv4.2 with one sample.  A target that is not split lists the edits of its consensus as\n"
            "                      RNAME POS . REF ALT . . PAIR=UNSPLIT;DP=span;AD=ref,alt GT 1/1.  A split target lists the edits\n"
            "                      of its two groups against the target, merged by position, GT:PS group 1 | group 2 with PS 1:\n"
            "                      PAIR=HOM 1|1 when both groups' consensus carry the same edit (written once), PAIR=HET 1|0 or 0|1\n"
            "                      when one does and the other covers the place, PAIR=CLASH 1|. and .|1 when the other carries a\n"
            "                      different edit that touches it (two records, not one 1|2), PAIR=NOCOV 1|. or .|1 when the other\n"
            "                      group has no consensus there; DP1=;AD1= and DP2=;AD2= are the read support in the edit's own\n"
            "                      group (unlabelled reads are in both).  Insertions and deletions are anchored as in --vcf; REF\n"
            "                      and ALT are not normalised and an allele has no length limit.  Turns on what it needs (the\n"
            "                      pile-up, the split, the second run, the edits and their support); the pairing runs on the GPU;\n"
            "                      stdout and every other file do not change.  Honours --site-min-*, --hap-min-*, --max-error and\n"
            "                      --max-depth.  Not with --window, -a, --polish.  This build's own rule, parity unpinned\n"
            "  --polish N          with -a: N more rounds, each with the previous round's consensus as the backbone the reads\n"
            "                      are re-aligned to (README.md:14-15 of the reference: 'the new consensus can be used as a new\n"
            "                      backbone sequence to iteratively improve the consensus quality')\n"
            "  --devices LIST      GPUs to use, e.g. 0,1,2,3 (default 0): one consensus worker per GPU, batches of\n"
            "                      targets dealt round-robin, records still printed in input order\n"
            "  --contexts N        consensus workers (thread + context) per GPU, 1..4: a batch's upload and formatting run\n"
            "                      beside another batch's kernels (default: 2 for inputs of several batches, else 1)\n"
            "  --link-sites        where --haplotag, --hap-consensus, --hap-sites and --hap-vcf go, and with --window --phase-windows\n"
            "                      where --site-reads, --haplotag, --hap-contigs and --hap-windows go: only the sites that the same\n"
            "                      reads carry as other sites near them sign the split.  Two sites of a target are partners when,\n"
            "                      of the reads with one of the two alleles at both, at most F disagree (--link-max-conflict,\n"
            "                      default 0.1, at most six decimal places) and the rarer agreeing combination is shown by N or\n"
            "                      more reads (--link-min-cell, default 3); a site is linked when it has N or more partners\n"
            "                      (--link-min-partners, default 2) among the N sites on either side of it in the target's site\n"
            "                      list (--link-reach, default 256, at most 4096).  At a site that is not linked no read counts\n"
            "                      as informative: HAP, SITES, the tally, H1 H2 H0 and everything else that rests on the split\n"
            "                      follow; the sites themselves, their reads and their alleles are listed as before.  A 0 means\n"
            "                      the default.  The defaults come from one experiment on synthetic reads (1 %% substitutions, 10 %%\n"
            "                      inserted and 4 %% deleted bases) and from nothing else.  Chosen on the GPU; stdout does not\n"
            "                      change.  This build's own rule, parity unpinned\n"
            "  --linked-sites FILE the same inputs, implies --link-sites: one line per site, RNAME POS PARTNERS LINKED, POS 1-based\n"
            "                      as in --sites, LINKED 1 or 0; with --window a position's line comes from the window whose core\n"
            "                      holds it\n"
            "  --hap-contigs FILE  with --window and --phase-windows (either this or --hap-windows stands in for --site-reads /\n"
            "                      --haplotag there): two phased sequences per phase block.  Every window whose reads split\n"
            "                      (--hap-min-sites, --hap-min-reads as for --hap-consensus) is run again as its two read groups,\n"
            "                      named in the block's orientation, and the groups' consensus is joined per label across the\n"
            "                      windows as the plain stitch joins the windows: a part continues the piece before it when both\n"
            "                      were cut at the core boundary between two neighbouring windows of one block.  An unsplit\n"
            "                      window, a failed one and a block boundary end both contigs.  FASTA, >RNAME/hap{1|2}/PS/t0_t1\n"
            "                      in target coordinates, PS as in --haplotag; records by t0, hap1 first; pieces shorter than -m\n"
            "                      are dropped.  The cut of every segment at its window's core is made on the GPU (16 bytes a\n"
            "                      segment come back, no per-base positions); stdout and every other file do not change.\n"
            "                      Honours --site-min-*, --hap-min-* and --phase-min-links / --phase-max-conflict.  Not with -a,\n"
            "                      --polish.  This build's own rule, parity unpinned\n"
            "  --hap-windows FILE  the same inputs: one line per window, #window RNAME BEGIN END PS N1 N2 N0 SEP AGREE DISAGREE SPLIT\n"
            "                      (the core, and the window's tally), then one line per site with a phase inside the core,\n"
            "                      RNAME POS PHASE P1 M1 P2 M2 with POS 1-based in target coordinates; all in the block's\n"
            "                      orientation (a flipped window's N1 / N2 and P1 M1 / P2 M2 change places, PHASE changes sign)\n"
            "  <input>             BLASR -m 5 file (.pre with -a, SAM with --sam, BAM with --bam, PAF with --paf) sorted by target, or - for stdin\n"
            "  version 0.3 (dagcon-mi355x)\n");
}

bool parse_uint(const char *s, unsigned *out) {
    char *e = nullptr;
    errno = 0;
    unsigned long v = strtoul(s, &e, 10);
    if (errno || !e || *e || v > 0xFFFFFFFFul) return false;
    *out = (unsigned)v;
    return true;
}

int parse_args(int argc, char **argv, Opts &o) {
    bool align = false, sam = false, bam = false, paf = false, cs = false, md = false;   // -a, --sam, --bam, --paf, --cs, --md as typed
    for (int i = 1; i < argc; i++) {
        std::string a = argv[i];
        auto need = [&](unsigned *dst) {
            if (i + 1 >= argc || !parse_uint(argv[i + 1], dst)) { fprintf(stderr, "PARSE ERROR: %s needs an unsigned integer\n", a.c_str()); return false; }
            i++;
            return true;
        };
        if (a == "-j" || a == "--threads") { if (!need(&o.threads)) return 2; }
        else if (a == "-c" || a == "--min-coverage") { if (!need(&o.min_cov)) return 2; }
        else if (a == "-m" || a == "--min-length") { if (!need(&o.min_len)) return 2; }
        else if (a == "-t" || a == "--trim") { if (!need(&o.trim)) return 2; }
        else if (a == "-a" || a == "--align") align = true;
        else if (a == "--local") o.local = true;
        else if (a == "--fastq") o.fastq = true;
        else if (a == "--sam") sam = true;
        else if (a == "--bam") bam = true;
        else if (a == "--paf") paf = true;
        else if (a == "--cs") cs = true;
        else if (a == "--md") md = true;
        else if (a == "--reads") {
            if (i + 1 >= argc) { fprintf(stderr, "PARSE ERROR: --reads needs a FASTA or FASTQ file\n"); return 2; }
            o.reads = argv[++i];
        }
        else if (a == "--edits") {
            if (i + 1 >= argc) { fprintf(stderr, "PARSE ERROR: --edits needs a file name\n"); return 2; }
            o.edits = argv[++i];
        }
        else if (a == "--vcf") {
            if (i + 1 >= argc) { fprintf(stderr, "PARSE ERROR: --vcf needs a file name\n"); return 2; }
            o.vcf = argv[++i];
        }
        else if (a == "--pileup") {
            if (i + 1 >= argc) { fprintf(stderr, "PARSE ERROR: --pileup needs a file name\n"); return 2; }
            o.pile.pileup = argv[++i];
        }
        else if (a == "--sites") {
            if (i + 1 >= argc) { fprintf(stderr, "PARSE ERROR: --sites needs a file name\n"); return 2; }
            o.pile.sites = argv[++i];
        }
        else if (a == "--site-reads") {
            if (i + 1 >= argc) { fprintf(stderr, "PARSE ERROR: --site-reads needs a file name\n"); return 2; }
            o.sr.site_reads = argv[++i];
        }
        else if (a == "--site-alleles") {
            if (i + 1 >= argc) { fprintf(stderr, "PARSE ERROR: --site-alleles needs a file name\n"); return 2; }
            o.al.alleles = argv[++i];
        }
        else if (a == "--site-vcf") {
            if (i + 1 >= argc) { fprintf(stderr, "PARSE ERROR: --site-vcf needs a file name\n"); return 2; }
            o.al.vcf = argv[++i];
        }
        else if (a == "--joined-alleles") {
            if (i + 1 >= argc) { fprintf(stderr, "PARSE ERROR: --joined-alleles needs a file name\n"); return 2; }
            o.jn.alleles = argv[++i];
        }
        else if (a == "--joined-vcf") {
            if (i + 1 >= argc) { fprintf(stderr, "PARSE ERROR: --joined-vcf needs a file name\n"); return 2; }
            o.jn.vcf = argv[++i];
        }
        else if (a == "--haplotag") {
            if (i + 1 >= argc) { fprintf(stderr, "PARSE ERROR: --haplotag needs a file name\n"); return 2; }
            o.sr.haplotag = argv[++i];
        }
        else if (a == "--hap-consensus") {
            if (i + 1 >= argc) { fprintf(stderr, "PARSE ERROR: --hap-consensus needs a file name\n"); return 2; }
            o.hap.consensus = argv[++i];
        }
        else if (a == "--hap-sites") {
            if (i + 1 >= argc) { fprintf(stderr, "PARSE ERROR: --hap-sites needs a file name\n"); return 2; }
            o.hap.sites = argv[++i];
        }
        else if (a == "--hap-vcf") {
            if (i + 1 >= argc) { fprintf(stderr, "PARSE ERROR: --hap-vcf needs a file name\n"); return 2; }
            o.hap.vcf = argv[++i];
        }
        else if (a == "--hap-contigs") {
            if (i + 1 >= argc) { fprintf(stderr, "PARSE ERROR: --hap-contigs needs a file name\n"); return 2; }
            o.hap_contigs = argv[++i];
        }
        else if (a == "--hap-windows") {
            if (i + 1 >= argc) { fprintf(stderr, "PARSE ERROR: --hap-windows needs a file name\n"); return 2; }
            o.hap_windows = argv[++i];
        }
        else if (a == "--link-sites") o.link.on = true;
        else if (a == "--linked-sites") {
            if (i + 1 >= argc) { fprintf(stderr, "PARSE ERROR: --linked-sites needs a file name\n"); return 2; }
            o.link.linked = argv[++i]; o.link.on = true;
        }
        else if (a == "--link-max-conflict") {
            if (i + 1 >= argc || !dg_parse_ppm(argv[i + 1], &o.link.o.max_conflict_ppm)) { fprintf(stderr, "PARSE ERROR: --link-max-conflict takes a fraction in [0, 1] with at most six decimal places\n"); return 2; }
            i++; o.link.opts_set = true;
        }
        else if (a == "--link-min-cell") { if (!need(&o.link.o.min_cell)) return 2; o.link.opts_set = true; }
        else if (a == "--link-min-partners") { if (!need(&o.link.o.min_partners)) return 2; o.link.opts_set = true; }
        else if (a == "--link-reach") {
            if (!need(&o.link.o.reach) || o.link.o.reach > 4096u) { fprintf(stderr, "PARSE ERROR: --link-reach takes 0..4096\n"); return 2; }
            o.link.opts_set = true;
        }
        else if (a == "--hap-min-sites") { if (!need(&o.hap.min_sites)) return 2; o.hap.sites_set = true; }
        else if (a == "--hap-min-reads") { if (!need(&o.hap.min_reads)) return 2; o.hap.reads_set = true; }
        else if (a == "--site-min-frac") {
            if (i + 1 >= argc || !dg_parse_ppm(argv[i + 1], &o.pile.min_frac_ppm)) { fprintf(stderr, "PARSE ERROR: --site-min-frac takes a fraction in [0, 1] with at most six decimal places\n"); return 2; }
            i++; o.pile.frac_set = true;
        }
        else if (a == "--site-min-count") { if (!need(&o.pile.min_count)) return 2; o.pile.count_set = true; }
        else if (a == "--phase-windows") o.wp.on = true;
        else if (a == "--phase-min-links") { if (!need(&o.wp.min_links)) return 2; o.wp.links_set = true; }
        else if (a == "--phase-max-conflict") {
            if (i + 1 >= argc || !dg_parse_ppm(argv[i + 1], &o.wp.max_conflict_ppm)) { fprintf(stderr, "PARSE ERROR: --phase-max-conflict takes a fraction in [0, 1] with at most six decimal places\n"); return 2; }
            i++; o.wp.conflict_set = true;
        }
        else if (a == "--window") { if (!need(&o.window) || !o.window) { fprintf(stderr, "PARSE ERROR: --window takes a positive number of bases\n"); return 2; } }
        else if (a == "--max-error") {
            if (i + 1 >= argc || !dg_parse_ppm(argv[i + 1], &o.pick.max_error_ppm)) { fprintf(stderr, "PARSE ERROR: --max-error takes a fraction in [0, 1] with at most six decimal places\n"); return 2; }
            i++; o.pick.error_set = true;
        }
        else if (a == "--max-depth") {
            if (!need(&o.pick.max_depth) || !o.pick.max_depth || o.pick.max_depth > DAGCON_MAX_COVERAGE) { fprintf(stderr, "PARSE ERROR: --max-depth takes 1..%u\n", DAGCON_MAX_COVERAGE); return 2; }
            o.pick.depth_set = true;
        }
        else if (a == "--overlap") { if (!need(&o.overlap)) return 2; o.overlap_set = true; }
        else if (a == "--ref") {
            if (i + 1 >= argc) { fprintf(stderr, "PARSE ERROR: --ref needs a FASTA file\n"); return 2; }
            o.ref = argv[++i];
        }
        else if (a == "-v" || a == "--verbose") o.verbose = true;
        else if (a == "--dump-parsed") o.dump = true;            // test hook: parser only, no GPU
        else if (a == "--slab-bytes") { unsigned v = 0; if (!need(&v)) return 2; o.slab_bytes = v; }   // test hook
        else if (a == "--batch-targets") { unsigned v = 0; if (!need(&v) || !v) return 2; o.batch_targets = v; }
        else if (a == "--polish") { if (!need(&o.polish)) return 2; }
        else if (a == "--contexts") { if (!need(&o.contexts) || !o.contexts || o.contexts > 4) { fprintf(stderr, "PARSE ERROR: --contexts takes 1..4\n"); return 2; } }
        else if (a == "--pinned") { unsigned v = 0; if (!need(&v)) return 2; o.pinned = v ? 1 : 0; }
        else if (a == "--devices") {
            if (i + 1 >= argc) { fprintf(stderr, "PARSE ERROR: --devices needs a list such as 0,1,2\n"); return 2; }
            o.devices.clear();
            const char *p = argv[++i];
            while (*p) {
                char *e = nullptr;
                const long v = strtol(p, &e, 10);
                if (e == p || v < 0 || v > 1023) { fprintf(stderr, "PARSE ERROR: bad --devices list\n"); return 2; }
                o.devices.push_back((int)v);
                p = *e == ',' ? e + 1 : e;
                if (*e && *e != ',') { fprintf(stderr, "PARSE ERROR: bad --devices list\n"); return 2; }
            }
            if (o.devices.empty()) { fprintf(stderr, "PARSE ERROR: --devices list is empty\n"); return 2; }
        }
        else if (a == "-h" || a == "--help") { usage(stdout); exit(0); }
        else if (a == "--version") { printf("pbdagcon  version: 0.3\n"); exit(0); }
        else if (a == "-" || a[0] != '-') {
            if (!o.input.empty()) { fprintf(stderr, "PARSE ERROR: more than one input\n"); return 2; }
            o.input = a;
        } else { fprintf(stderr, "PARSE ERROR: unknown argument %s\n", a.c_str()); return 2; }
    }
    if (o.local && !align) { fprintf(stderr, "PARSE ERROR: --local needs -a\n"); return 2; }
    if (md && !sam && !bam) { fprintf(stderr, "PARSE ERROR: --md needs --sam or --bam\n"); return 2; }
    if (md && !o.ref.empty()) { fprintf(stderr, "PARSE ERROR: --md does not go with --ref (the MD:Z: tags stand in for the FASTA)\n"); return 2; }
    if (md && (paf || align || o.local || o.polish)) { fprintf(stderr, "PARSE ERROR: --md does not go with --paf, -a, --local or --polish\n"); return 2; }
    if (cs && !paf) { fprintf(stderr, "PARSE ERROR: --cs needs --paf\n"); return 2; }
    if (cs && !o.reads.empty()) { fprintf(stderr, "PARSE ERROR: --cs does not go with --reads (a cs:Z: tag and --ref are the whole alignment)\n"); return 2; }
    if (cs && (sam || bam || align || o.local || o.polish)) { fprintf(stderr, "PARSE ERROR: --cs does not go with --sam, --bam, -a, --local or --polish\n"); return 2; }
    if (paf && (sam || bam)) { fprintf(stderr, "PARSE ERROR: --paf does not go with --sam or --bam\n"); return 2; }
    if (paf && (align || o.local || o.polish)) { fprintf(stderr, "PARSE ERROR: --paf does not go with -a, --local or --polish\n"); return 2; }
    if (paf && o.ref.empty()) { fprintf(stderr, "PARSE ERROR: --paf needs --ref <fasta>\n"); return 2; }
    if (paf && !cs && o.reads.empty()) { fprintf(stderr, "PARSE ERROR: --paf needs --reads <fasta|fastq>\n"); return 2; }
    if (!paf && !o.reads.empty()) { fprintf(stderr, "PARSE ERROR: --reads needs --paf\n"); return 2; }
    if (bam && sam) { fprintf(stderr, "PARSE ERROR: --bam and --sam do not go together\n"); return 2; }
    if (bam && (align || o.local || o.polish)) { fprintf(stderr, "PARSE ERROR: --bam does not go with -a, --local or --polish\n"); return 2; }
    if (bam && o.ref.empty() && !md) { fprintf(stderr, "PARSE ERROR: --bam needs --ref <fasta>\n"); return 2; }
    const bool records = sam || bam || paf;
    if (sam && (align || o.local || o.polish)) { fprintf(stderr, "PARSE ERROR: --sam does not go with -a, --local or --polish\n"); return 2; }
    if (sam && o.ref.empty() && !md) { fprintf(stderr, "PARSE ERROR: --sam needs --ref <fasta>\n"); return 2; }
    if (!records && !o.ref.empty()) { fprintf(stderr, "PARSE ERROR: --ref needs --sam, --bam or --paf\n"); return 2; }
    if (o.window && (!records || align || o.polish)) { fprintf(stderr, "PARSE ERROR: --window needs --sam, --bam or --paf and does not go with -a or --polish\n"); return 2; }
    if (o.pick.on() && !records) { fprintf(stderr, "PARSE ERROR: --max-error and --max-depth need --sam, --bam or --paf\n"); return 2; }
    if (!o.edits.empty() && !records) { fprintf(stderr, "PARSE ERROR: --edits needs --sam, --bam or --paf\n"); return 2; }
    if (!o.edits.empty() && o.dump) { fprintf(stderr, "PARSE ERROR: --edits does not go with --dump-parsed (nothing is run, the file would not be written)\n"); return 2; }
    if (!o.vcf.empty() && !records) { fprintf(stderr, "PARSE ERROR: --vcf needs --sam, --bam or --paf\n"); return 2; }
    if (!o.vcf.empty() && o.dump) { fprintf(stderr, "PARSE ERROR: --vcf does not go with --dump-parsed (nothing is run, the file would not be written)\n"); return 2; }
    if (!o.vcf.empty() && o.window) { fprintf(stderr, "PARSE ERROR: --vcf does not go with --window (the stitch splits and fuses edits: a fused edit has no single count)\n"); return 2; }
    if (o.want_hc() && (!o.window || !o.wp.on || align || o.polish)) { fprintf(stderr, "PARSE ERROR: --hap-contigs and --hap-windows need --window and --phase-windows and do not go with -a or --polish\n"); return 2; }
    if (o.want_hc() && o.dump) { fprintf(stderr, "PARSE ERROR: --hap-contigs and --hap-windows do not go with --dump-parsed (nothing is run, the files would not be written)\n"); return 2; }
    if ((o.pile.frac_set || o.pile.count_set) && o.pile.sites.empty() && !o.want_sr() && !o.want_hc()) { fprintf(stderr, "PARSE ERROR: --site-min-frac and --site-min-count need --sites\n"); return 2; }
    if (!o.hap.vcf.empty() && !records) { fprintf(stderr, "PARSE ERROR: --hap-vcf needs --sam, --bam or --paf (REF comes from the target's bases)\n"); return 2; }
    if ((o.hap.sites_set || o.hap.reads_set) && !o.hap.on() && !o.want_hc()) { fprintf(stderr, "PARSE ERROR: --hap-min-sites and --hap-min-reads need --hap-consensus or --hap-sites\n"); return 2; }
    if (o.hap.on() && (o.window || align || o.polish)) { fprintf(stderr, "PARSE ERROR: --hap-consensus and --hap-sites do not go with --window, -a or --polish (the groups of neighbouring windows are named each on its own)\n"); return 2; }
    if (o.hap.on() && o.dump) { fprintf(stderr, "PARSE ERROR: --hap-consensus and --hap-sites do not go with --dump-parsed (nothing is run, the files would not be written)\n"); return 2; }
    if (o.link.opts_set && !o.link.on) { fprintf(stderr, "PARSE ERROR: --link-max-conflict, --link-min-cell, --link-min-partners and --link-reach need --link-sites or --linked-sites\n"); return 2; }
    if (o.link.on && !(o.window ? o.wp.on : o.want_phase())) { fprintf(stderr, "PARSE ERROR: --link-sites and --linked-sites need --haplotag, --hap-consensus, --hap-sites or --hap-vcf (with --window: --phase-windows)\n"); return 2; }
    if (o.link.on && o.dump) { fprintf(stderr, "PARSE ERROR: --link-sites and --linked-sites do not go with --dump-parsed (nothing is run, the file would not be written)\n"); return 2; }
    if (o.wp.on && !o.window) { fprintf(stderr, "PARSE ERROR: --phase-windows needs --window\n"); return 2; }
    if (o.wp.on && !o.sr.on() && !o.want_hc()) { fprintf(stderr, "PARSE ERROR: --phase-windows needs --site-reads FILE or --haplotag FILE\n"); return 2; }
    if ((o.wp.links_set || o.wp.conflict_set) && !o.wp.on) { fprintf(stderr, "PARSE ERROR: --phase-min-links and --phase-max-conflict need --phase-windows\n"); return 2; }
    if (o.sr.on() && ((o.window && !o.wp.on) || align || o.polish)) { fprintf(stderr, "PARSE ERROR: --site-reads and --haplotag do not go with --window, -a or --polish (the groups of neighbouring windows are named each on its own)\n"); return 2; }
    if (o.sr.on() && o.dump) { fprintf(stderr, "PARSE ERROR: --site-reads and --haplotag do not go with --dump-parsed (nothing is run, the files would not be written)\n"); return 2; }
    if (o.al.on() && (o.window || align || o.polish)) { fprintf(stderr, "PARSE ERROR: --site-alleles and --site-vcf do not go with --window, -a or --polish (they go where --site-reads goes)\n"); return 2; }
    if (o.al.on() && o.dump) { fprintf(stderr, "PARSE ERROR: --site-alleles and --site-vcf do not go with --dump-parsed (nothing is run, the files would not be written)\n"); return 2; }
    if (!o.al.vcf.empty() && !records) { fprintf(stderr, "PARSE ERROR: --site-vcf needs --sam, --bam or --paf (REF comes from the target's bases)\n"); return 2; }
    if (o.jn.on() && (o.window || align || o.polish)) { fprintf(stderr, "PARSE ERROR: --joined-alleles and --joined-vcf do not go with --window, -a or --polish (they go where --site-reads goes)\n"); return 2; }
    if (o.jn.on() && o.dump) { fprintf(stderr, "PARSE ERROR: --joined-alleles and --joined-vcf do not go with --dump-parsed (nothing is run, the files would not be written)\n"); return 2; }
    if (!o.jn.vcf.empty() && !records) { fprintf(stderr, "PARSE ERROR: --joined-vcf needs --sam, --bam or --paf (REF comes from the target's bases)\n"); return 2; }
    if (o.pile.on() && o.polish) { fprintf(stderr, "PARSE ERROR: --pileup and --sites do not go with --polish (the backbone changes under the positions)\n"); return 2; }
    if (o.pile.on() && o.dump) { fprintf(stderr, "PARSE ERROR: --pileup and --sites do not go with --dump-parsed (nothing is run, the files would not be written)\n"); return 2; }
    if (o.overlap_set && !o.window) { fprintf(stderr, "PARSE ERROR: --overlap needs --window\n"); return 2; }
    if (o.window && (uint64_t)o.overlap < (uint64_t)o.trim + 64) { fprintf(stderr, "PARSE ERROR: --overlap must be at least --trim + 64 (%u)\n", o.trim + 64); return 2; }
    if (o.input.empty()) { fprintf(stderr, "PARSE ERROR: required argument missing: input\n"); usage(stderr); return 2; }
    o.mode = records ? MODE_RECORDS : align ? MODE_PRE : MODE_M5;
    o.kind = cs ? DG_REC_CS : paf ? DG_REC_STRANDED : bam ? (md ? DG_REC_PACKED_MD : DG_REC_PACKED) : md ? DG_REC_PLAIN_MD : DG_REC_PLAIN;
    return 0;
}

// Alignment.cpp:15-26: only upper-case ACGT are complemented, then the string is reversed
void revcomp_into(char *dst, const char *s, size_t n) {
    for (size_t i = 0; i < n; i++) {
        char c = s[n - 1 - i];
        dst[i] = c == 'T' ? 'A' : c == 'G' ? 'C' : c == 'A' ? 'T' : c == 'C' ? 'G' : c;
    }
}

// istringstream >> uint32_t on a token (Alignment.cpp:63-66)
uint32_t tok_u32(const char *s, size_t n) {
    uint64_t v = 0;
    size_t i = 0;
    bool any = false, over = false, neg = false;
    if (i < n && (s[i] == '+' || s[i] == '-')) { neg = s[i] == '-'; i++; }
    for (; i < n && s[i] >= '0' && s[i] <= '9'; i++) {
        if (!over) v = v * 10 + (uint64_t)(s[i] - '0');
        if (v > 0xFFFFFFFFull) over = true;
        any = true;
    }
    if (!any) return 0;
    if (over) return 0xFFFFFFFFu;
    return neg ? (uint32_t)(0u - (uint32_t)v) : (uint32_t)v;
}

// f(0) here and f(1) .. f(n - 1) on threads of their own
template <class F>
void on_threads(unsigned n, F f) {
    std::vector<std::thread> th;
    for (unsigned k = 1; k < n; k++) th.emplace_back(f, k);
    f(0);
    for (auto &x : th) x.join();
}

// string blob of a batch: page-locked (dagcon_host_alloc) when a context offers it, else malloc
struct Blob {
    char *p = nullptr;
    size_t cap = 0, n = 0;
    dagcon_ctx *owner = nullptr;       // context the page-locked block came from (nullptr: malloc)
    void release() {
        if (p) { if (owner) dagcon_host_free(owner, p); else free(p); }
        p = nullptr; cap = 0; owner = nullptr;
    }
    bool resize(size_t bytes, dagcon_ctx *pin) {
        if (bytes > cap) {
            release();
            const size_t want = bytes + bytes / 8 + 4096;
            void *q = nullptr;
            if (pin && dagcon_host_alloc(pin, want, &q) == DAGCON_OK) { p = (char *)q; owner = pin; }
            else { p = (char *)malloc(want); owner = nullptr; }
            if (!p) return false;
            cap = want;
        }
        n = bytes;
        return true;
    }
    char *data() { return p; }
    size_t size() const { return n; }
};

// The targets of one trip to the device.  .m5 / .pre: off2 / len2 are a record's target string in t.  Records: t holds each
// target's bases once (toff; tsrc: where they come from), ops every record's ops (from opb), cs_len / tspan what the cs kind adds
struct Batch {
    std::vector<std::string> ids;
    std::vector<uint32_t> tlen, start, len, len2;
    std::vector<uint64_t> begin{0}, off, off2;
    std::vector<char> strand;
    std::vector<uint64_t> toff, opb{0};
    std::vector<const char *> tsrc;
    std::vector<uint32_t> ops, cs_len, tspan;
    std::vector<uint8_t> reverse;
    std::vector<uint64_t> md_off;      // md kinds: every record's MD:Z: text in md
    std::vector<uint32_t> md_len;
    std::string md;
    Blob q, t;
    unsigned long long seq = 0;        // position in the input: records are printed in this order
    std::string out;                   // the batch's FASTA records
    std::string edits;                 // --edits: the batch's lines of that file
    unsigned long long n_edits = 0;
    std::string vcf, contigs;          // --vcf: the batch's lines of that file, and its targets' ##contig lines
    std::string pileup, sites;         // --pileup, --sites: the batch's lines of those files
    std::vector<std::string> qnames;   // --site-reads, --haplotag: the records' read names (the input's pages may be gone by the time they are written)
    std::string site_reads, haplotag;  // and the batch's lines of those files
    std::string hap_out, hap_sites;    // --hap-consensus, --hap-sites: the batch's records and lines of those files
    std::string linked_sites;          // --linked-sites: the batch's lines of that file
    std::string hap_vcf, hap_contigs;  // --hap-vcf: the batch's lines of that file, and its targets' ##contig lines
    std::string site_alleles, site_vcf, site_contigs;   // --site-alleles, --site-vcf: the batch's lines of those files, and its targets' ##contig lines
    std::string joined_alleles, joined_vcf, joined_contigs;   // --joined-alleles, --joined-vcf: the same
    void clear() { ids.clear(); tlen.clear(); start.clear(); len.clear(); len2.clear(); begin.assign(1, 0); off.clear(); off2.clear(); strand.clear(); toff.clear(); opb.assign(1, 0); tsrc.clear(); ops.clear(); cs_len.clear(); tspan.clear(); reverse.clear(); md_off.clear(); md_len.clear(); md.clear(); q.n = 0; t.n = 0; out.clear(); edits.clear(); n_edits = 0; vcf.clear(); contigs.clear(); pileup.clear(); sites.clear(); qnames.clear(); site_reads.clear(); haplotag.clear(); hap_out.clear(); hap_sites.clear(); linked_sites.clear(); hap_vcf.clear(); hap_contigs.clear(); site_alleles.clear(); site_vcf.clear(); site_contigs.clear(); joined_alleles.clear(); joined_vcf.clear(); joined_contigs.clear(); }
};

FILE *g_edits = nullptr;                                  // --edits FILE, written batch by batch in output order
unsigned long long g_n_edits = 0;
// --vcf FILE, opened before the workers start.  The header names every target, so the lines go to an unnamed temporary
// file batch by batch, in output order, and only the ##contig lines are kept; the end of the run writes header and lines
FILE *g_vcf = nullptr, *g_vcf_lines = nullptr;
std::string g_vcf_contigs;
bool g_vcf_bad = false;
FILE *g_pileup = nullptr, *g_sites = nullptr;              // --pileup FILE, --sites FILE, written batch by batch in output order
FILE *g_site_reads = nullptr, *g_haplotag = nullptr;       // --site-reads FILE, --haplotag FILE, the same way
FILE *g_hap_out = nullptr, *g_hap_sites = nullptr;         // --hap-consensus FILE, --hap-sites FILE, the same way
FILE *g_linked_sites = nullptr;                            // --linked-sites FILE, the same way
FILE *g_hap_contigs = nullptr, *g_hap_windows = nullptr;   // --hap-contigs FILE, --hap-windows FILE, the same way
FILE *g_hap_vcf = nullptr, *g_hap_vcf_lines = nullptr;     // --hap-vcf FILE, as --site-vcf below: the records wait in an unnamed temporary file
std::string g_hap_vcf_contigs;
FILE *g_site_alleles = nullptr;                            // --site-alleles FILE, the same way
// --site-vcf FILE, as --vcf: the header names every target, so the records wait in an unnamed temporary file
FILE *g_site_vcf = nullptr, *g_site_vcf_lines = nullptr;
std::string g_site_vcf_contigs;
FILE *g_joined_alleles = nullptr;                          // --joined-alleles FILE and --joined-vcf FILE, as those two
FILE *g_joined_vcf = nullptr, *g_joined_vcf_lines = nullptr;
std::string g_joined_vcf_contigs;
bool g_pile_bad = false;
unsigned long long g_over_error = 0, g_over_depth = 0;     // records --max-error / --max-depth left out, all batches (under g_tmu)
bool g_timing = false;                                    // PBDAGCON_TIMING=1: where the wall time of the run went, on stderr (seconds)
std::mutex g_tmu;
double g_t_upload = 0, g_t_run = 0, g_t_fetch = 0;
double wall() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// ---- one batch through the device, by mode ---------------------------------------------------------------------------

// false, with the library's message, when a call failed
bool ok(dagcon_ctx *ctx, int rc, const char *what) {
    if (rc != DAGCON_OK) fprintf(stderr, "pbdagcon: %s failed (%d): %s\n", what, rc, dagcon_last_error(ctx));
    return rc == DAGCON_OK;
}

// --hap-sites, --hap-consensus: the tally's lines; then the second run on the same context, from what the first left on
// the device, and its records.  What the first run's fetches point at is gone after dagcon_upload_haps
// one target's (one group's) edits [seg_begin[g], seg_begin[g + 1]) of a fetch as --hap-vcf writes them; hc NULL: unsplit,
// else the group's states, and each mate as an index into the partner's edits, which begin at mate0
std::vector<DgHapVcfEdit> hap_vcf_edits(const dagcon_results &r, const dagcon_edits &ed, const dagcon_edit_support &es, const uint32_t g,
                                        const dagcon_hap_calls *hc, const uint64_t mate0) {
    std::vector<DgHapVcfEdit> out;
    for (uint64_t e = ed.edit_begin[r.seg_begin[g]]; e < ed.edit_begin[r.seg_begin[g + 1]]; e++)
        out.push_back({ed.t_pos[e], ed.t_len[e], std::string(r.seq_blob + ed.c_off[e], ed.c_len[e]), es.span[e], es.ref[e], es.alt[e],
                       hc ? hc->state[e] : 0u, hc && hc->mate[e] != UINT64_MAX ? (long long)(hc->mate[e] - mate0) : -1ll});
    return out;
}

int append_haps(dagcon_ctx *ctx, Batch &b, const Opts &o, const dagcon_results &r1, const dagcon_edits &ed1, const dagcon_edit_support &es1,
                const dagcon_pileup_sites &ps, const dagcon_site_reads &sr) {
    dagcon_hap_tally ht;
    memset(&ht, 0, sizeof ht);
    if (!ok(ctx, dagcon_fetch_hap_tally(ctx, &ht), "tally of the split")) return 1;
    if (!o.hap.sites.empty())
        for (uint32_t g = 0; g < ht.n_targets; g++) {
            dg_hap_target_line(b.hap_sites, b.ids[g], ht.n1[g], ht.n2[g], ht.n0[g], ht.n_sep[g], ht.agree[g], ht.disagree[g], ht.split[g]);
            for (uint64_t s = ps.site_begin[g]; s < ps.site_begin[g + 1]; s++)
                if (sr.phase[s]) dg_hap_site_line(b.hap_sites, b.ids[g], ps.pos[s], sr.phase[s], ht.site_counts + 4 * s);
        }
    if (o.hap.consensus.empty() && o.hap.vcf.empty()) return 0;
    // --hap-vcf: an unsplit target's lines are the first run's own edits, taken here, before the second run takes their place
    std::vector<std::string> vcf_lines(o.hap.vcf.empty() ? 0 : ht.n_targets);
    for (uint32_t g = 0; g < vcf_lines.size(); g++) {
        dg_vcf_contig(b.hap_contigs, b.ids[g], b.tlen[g]);
        if (!ht.split[g] && r1.target_status[g] == DAGCON_OK)
            dg_hap_vcf_unsplit(vcf_lines[g], b.ids[g], b.t.data() + b.toff[g], b.tlen[g], hap_vcf_edits(r1, ed1, es1, g, nullptr, 0));
    }
    dagcon_results r;
    dagcon_hap_map hm;
    int rc = dagcon_upload_haps(ctx);
    if (rc == DAGCON_OK) rc = dagcon_run(ctx);
    if (rc == DAGCON_OK) rc = dagcon_fetch(ctx, &r);
    if (rc == DAGCON_OK) rc = dagcon_fetch_hap_map(ctx, &hm);
    if (!ok(ctx, rc, "consensus per group")) return 1;
    for (uint32_t g = 0; g < r.n_targets; g++) {
        const std::string id = dg_hap_id(b.ids[hm.src_target[g]], hm.label[g]);
        if (r.target_status[g] != DAGCON_OK)
            fprintf(stderr, "pbdagcon: warning: group %s skipped (%s)\n", id.c_str(), dg_status_text(r.target_status[g], "an alignment leaves the backbone or holds a non-printable byte"));
        for (uint64_t s = r.seg_begin[g]; s < r.seg_begin[g + 1]; s++)
            if (!o.hap.consensus.empty() && !dg_append_result(b.hap_out, false, id, r.range0[s], r.range1[s], r.seq_blob + r.seq_off[s], r.seq_len[s], nullptr, nullptr)) return 1;
    }
    if (o.hap.vcf.empty()) return 0;
    // a split target's lines: the edits of its two groups, label 1 at d and label 2 at d + 1, with their support and states
    dagcon_edits ed;
    dagcon_edit_support es;
    dagcon_hap_calls hc;
    rc = dagcon_fetch_edits(ctx, &ed);
    if (rc == DAGCON_OK) rc = dagcon_fetch_edit_support(ctx, &es);
    if (rc == DAGCON_OK) rc = dagcon_fetch_hap_calls(ctx, &hc);
    if (!ok(ctx, rc, "hap calls")) return 1;
    for (uint32_t d = 0; d + 1 < r.n_targets; d += 2) {
        const uint32_t g = hm.src_target[d];
        const uint64_t b1 = ed.edit_begin[r.seg_begin[d]], b2 = ed.edit_begin[r.seg_begin[d + 1]];
        dg_hap_vcf_split(vcf_lines[g], b.ids[g], b.t.data() + b.toff[g], b.tlen[g], hap_vcf_edits(r, ed, es, d, &hc, b2), hap_vcf_edits(r, ed, es, d + 1, &hc, b1));
    }
    for (const std::string &x : vcf_lines) b.hap_vcf += x;
    return 0;
}

// the records of the results to b.out (main.cpp:141-143), warnings to stderr
int append_results(dagcon_ctx *ctx, Batch &b, const Opts &o, const dagcon_results &r) {
    dagcon_support sup;
    memset(&sup, 0, sizeof sup);
    if (o.fastq && !ok(ctx, dagcon_fetch_support(ctx, &sup), "per-base support")) return 1;
    dagcon_edits ed;
    memset(&ed, 0, sizeof ed);
    if (o.want_edits() && !ok(ctx, dagcon_fetch_edits(ctx, &ed), "edits")) return 1;
    dagcon_edit_support es;
    memset(&es, 0, sizeof es);
    if (o.want_edit_support() && !ok(ctx, dagcon_fetch_edit_support(ctx, &es), "edit support")) return 1;
    dagcon_pileup pu;
    memset(&pu, 0, sizeof pu);
    if (!o.pile.pileup.empty() && !ok(ctx, dagcon_fetch_pileup(ctx, &pu), "pile-up")) return 1;
    dagcon_pileup_sites ps;
    memset(&ps, 0, sizeof ps);
    if ((!o.pile.sites.empty() || o.want_sr()) && !ok(ctx, dagcon_fetch_pileup_sites(ctx, &ps), "pile-up sites")) return 1;
    dagcon_site_reads sr;
    memset(&sr, 0, sizeof sr);
    if (o.want_sr() && !ok(ctx, dagcon_fetch_site_reads(ctx, &sr), "site reads")) return 1;
    dagcon_site_link sl;
    memset(&sl, 0, sizeof sl);
    if (o.link.on && !ok(ctx, dagcon_fetch_site_link(ctx, &sl), "site link")) return 1;
    dagcon_site_alleles sa;
    memset(&sa, 0, sizeof sa);
    if (o.want_al() && !ok(ctx, dagcon_fetch_site_alleles(ctx, &sa), "site alleles")) return 1;
    dagcon_joined_sites js;
    memset(&js, 0, sizeof js);
    if (o.jn.on() && !ok(ctx, dagcon_fetch_joined_sites(ctx, &js), "joined sites")) return 1;
    uint64_t sr_x = 0;                                      // (aln_tgt ascends: one walk over the taken alignments)
    const char *nonconforming = o.mode == MODE_RECORDS ? dg_kind(o.kind).nonconforming : "an alignment leaves the backbone or holds a non-printable byte";
    for (uint32_t g = 0; g < r.n_targets; g++) {
        if (o.verbose)
            fprintf(stderr, "Consensus calling: %s Alignments: %llu\n", b.ids[g].c_str(),
                    (unsigned long long)(b.begin[g + 1] - b.begin[g]));
        // a failure is confined to its target (the reference's assert hits one worker's one target,
        // AlnGraphBoost.cpp:71-72): warn, go on with the rest
        if (!o.vcf.empty()) dg_vcf_contig(b.contigs, b.ids[g], b.tlen[g]);
        if (o.pile.on()) {
            // REF: the record inputs carry the target's bases (--md: as the device rebuilt them, run_records)
            const char *tb = o.mode == MODE_RECORDS ? b.t.data() + b.toff[g] : nullptr;
            if (!o.pile.pileup.empty()) dg_pileup_lines(b.pileup, b.ids[g], pu, g, 0, b.tlen[g], 0, tb);
            if (!o.pile.sites.empty()) dg_site_lines(b.sites, b.ids[g], ps, g, 0, b.tlen[g], 0, tb);
        }
        if (o.sr.on()) {
            const uint64_t x0 = sr_x;
            while (sr_x < sr.n_aln && sr.aln_tgt[sr_x] == g) sr_x++;
            dg_site_read_lines(o.sr.site_reads.empty() ? nullptr : &b.site_reads, o.sr.haplotag.empty() ? nullptr : &b.haplotag, b.ids[g], ps, sr, g, x0, sr_x, b.qnames, o.link.on ? sl.linked : nullptr);
        }
        if (!o.link.linked.empty()) dg_linked_site_lines(b.linked_sites, b.ids[g], ps, sl, g, 0, b.tlen[g], 0);
        if (o.al.on()) {
            const char *tb = o.mode == MODE_RECORDS ? b.t.data() + b.toff[g] : nullptr;
            if (!o.al.vcf.empty()) dg_vcf_contig(b.site_contigs, b.ids[g], b.tlen[g]);
            dg_site_allele_lines(o.al.alleles.empty() ? nullptr : &b.site_alleles, o.al.vcf.empty() ? nullptr : &b.site_vcf, b.ids[g], ps, sa, g, tb, b.tlen[g], o.pile.min_count);
        }
        if (o.jn.on()) {
            const char *tb = o.mode == MODE_RECORDS ? b.t.data() + b.toff[g] : nullptr;
            if (!o.jn.vcf.empty()) dg_vcf_contig(b.joined_contigs, b.ids[g], b.tlen[g]);
            dg_joined_lines(o.jn.alleles.empty() ? nullptr : &b.joined_alleles, o.jn.vcf.empty() ? nullptr : &b.joined_vcf, b.ids[g], ps, sa, js, g, tb, b.tlen[g], o.pile.min_count);
        }
        if (r.target_status[g] != DAGCON_OK)
            fprintf(stderr, "pbdagcon: warning: target %s skipped (%s)\n", b.ids[g].c_str(), dg_status_text(r.target_status[g], nonconforming));
        for (uint64_t s = r.seg_begin[g]; s < r.seg_begin[g + 1]; s++) {
            if (!dg_append_result(b.out, o.fastq, b.ids[g], r.range0[s], r.range1[s], r.seq_blob + r.seq_off[s], r.seq_len[s],
                                  o.fastq ? sup.weight + r.seq_off[s] : nullptr, o.fastq ? sup.depth + r.seq_off[s] : nullptr)) return 1;
            if (!o.vcf.empty())
                for (uint64_t e = ed.edit_begin[s]; e < ed.edit_begin[s + 1]; e++)
                    dg_vcf_line(b.vcf, b.ids[g], b.t.data() + b.toff[g], b.tlen[g], ed.t_pos[e], ed.t_len[e], r.seq_blob + ed.c_off[e], ed.c_len[e],
                                es.span[e], es.ref[e], es.alt[e], es.w_begin[e], es.w_end[e]);
            if (o.edits.empty()) continue;
            // the record's span and edits (include/dagcon.h, dagcon_edits): REF from the target's bases, ALT from the record's
            char head[64];
            snprintf(head, sizeof head, " %u %u\n", ed.seg_t0[s], ed.seg_t1[s]);
            b.edits += "#piece "; b.edits += b.ids[g]; b.edits += head;
            const char *tb = b.t.data() + b.toff[g];
            for (uint64_t e = ed.edit_begin[s]; e < ed.edit_begin[s + 1]; e++) {
                snprintf(head, sizeof head, "\t%u\t%u\t", ed.t_pos[e], ed.t_pos[e] + ed.t_len[e]);
                b.edits += b.ids[g]; b.edits += head;
                if (ed.t_len[e]) b.edits.append(tb + ed.t_pos[e], ed.t_len[e]); else b.edits += '-';
                b.edits += '\t';
                if (ed.c_len[e]) b.edits.append(r.seq_blob + ed.c_off[e], ed.c_len[e]); else b.edits += '-';
                b.edits += '\n';
            }
            b.n_edits += ed.edit_begin[s + 1] - ed.edit_begin[s];
        }
    }
    return o.hap.on() ? append_haps(ctx, b, o, r, ed, es, ps, sr) : 0;  // (last: the second run takes the place of everything above)
}

// the batch's own strings as the library's batch
dagcon_batch strings_batch(Batch &b) {
    dagcon_batch db;
    memset(&db, 0, sizeof db);
    db.n_targets = (uint32_t)b.ids.size();
    db.tlen = b.tlen.data(); db.aln_begin = b.begin.data();
    db.aln_start = b.start.data(); db.aln_off = b.off.data(); db.aln_len = b.len.data();
    db.qstr = b.q.data(); db.tstr = b.t.data(); db.blob_bytes = b.q.size();
    return db;
}

// dagcon_consensus; with PBDAGCON_TIMING its three steps, timed apart
bool consensus_strings(dagcon_ctx *ctx, const dagcon_batch &db, dagcon_results &r) {
    int rc;
    if (g_timing) {
        const double t0 = wall();
        rc = dagcon_upload(ctx, &db);
        const double t1 = wall();
        if (rc == DAGCON_OK) rc = dagcon_run(ctx);
        if (rc == DAGCON_OK) rc = dagcon_sync(ctx);
        const double t2 = wall();
        if (rc == DAGCON_OK) rc = dagcon_fetch(ctx, &r);
        const double t3 = wall();
        std::lock_guard<std::mutex> lk(g_tmu);
        g_t_upload += t1 - t0; g_t_run += t2 - t1; g_t_fetch += t3 - t2;
    } else rc = dagcon_consensus(ctx, &db, &r);
    return ok(ctx, rc, "consensus");
}

// plain .m5: the strings as they were parsed
int run_m5(dagcon_ctx *ctx, Batch &b, const Opts &o) {
    dagcon_results r;
    return consensus_strings(ctx, strings_batch(b), r) ? append_results(ctx, b, o, r) : 1;
}

// position + read + CIGAR (cs kind: cs text) per record, the target's bases once: expanded on the device
int run_records(dagcon_ctx *ctx, Batch &b, const Opts &o) {
    DgRecordArrays ra{};
    ra.cb.n_targets = (uint32_t)b.ids.size(); ra.cb.tlen = b.tlen.data(); ra.cb.t_off = b.toff.data();
    ra.cb.t_blob = b.t.data(); ra.cb.t_bytes = b.t.size(); ra.cb.rec_begin = b.begin.data();
    ra.cb.pos = b.start.data(); ra.cb.q_off = b.off.data(); ra.cb.q_len = b.len.data();
    ra.cb.q_blob = b.q.data(); ra.cb.q_bytes = b.q.size(); ra.cb.op_begin = b.opb.data(); ra.cb.ops = b.ops.data();
    ra.reverse = o.kind == DG_REC_STRANDED ? b.reverse.data() : nullptr; ra.cs_len = b.cs_len.data(); ra.t_span = b.tspan.data();
    if (dg_kind_md(o.kind)) {                               // (b.t is not read: the device makes the targets)
        ra.cb.t_blob = nullptr;
        ra.md.md_off = b.md_off.data(); ra.md.md_len = b.md_len.data(); ra.md.md_blob = b.md.data(); ra.md.md_bytes = b.md.size();
    }
    dagcon_results r;
    const double t0 = wall();
    const int rc = dg_consensus_records(ctx, o.kind, ra, nullptr, &r);
    if (g_timing) fprintf(stderr, "pbdagcon timing: %s%s batch of %zu records: %s %.3f\n", dg_kind(o.kind).flag, o.pick.text().c_str(), b.start.size(), dg_kind(o.kind).entry, wall() - t0);
    if (!ok(ctx, rc, "consensus")) return 1;
    if (dg_kind_md(o.kind) && (o.want_edits() || o.pile.on() || o.want_al())) {   // REF of the edits, of the pile-up lines and of the alleles' lines and records: the targets as the device rebuilt them, in b.t's layout
        const char *tb = nullptr;
        uint64_t tn = 0;
        if (!ok(ctx, dagcon_fetch_md_targets(ctx, &tb, &tn), "rebuilt targets")) return 1;
        memcpy(b.t.data(), tb, std::min<uint64_t>(tn, b.t.size()));
    }
    uint64_t n_fate = 0;
    if (const uint8_t *fate = dg_record_fates(ctx, &n_fate)) {
        unsigned long long over_error = 0, over_depth = 0;
        for (uint64_t i = 0; i < n_fate; i++) { over_error += (fate[i] & DAGCON_FATE_MAX_ERROR) != 0; over_depth += (fate[i] & DAGCON_FATE_MAX_DEPTH) != 0; }
        std::lock_guard<std::mutex> lk(g_tmu);
        g_over_error += over_error; g_over_depth += over_depth;
    }
    return append_results(ctx, b, o, r);
}

void warn_dropped(dagcon_ctx *ctx, size_t n_records) {
    if (const uint32_t nd = dagcon_align_dropped(ctx)) fprintf(stderr, "pbdagcon: warning: %u of %zu records could not be aligned inside the widest band and were dropped\n", nd, n_records);
}

// -a: SimpleAligner on every record first (main.cpp:117-145), in one call: the aligned strings stay on the device
int run_pre(dagcon_ctx *ctx, Batch &b, const Opts &o) {
    dagcon_pre_batch pb;
    memset(&pb, 0, sizeof pb);
    pb.n_targets = (uint32_t)b.ids.size(); pb.tlen = b.tlen.data(); pb.rec_begin = b.begin.data();
    pb.tstart = b.start.data(); pb.strand = b.strand.data();
    pb.q_off = b.off.data(); pb.q_len = b.len.data(); pb.t_off = b.off2.data(); pb.t_len = b.len2.data();
    pb.q_blob = b.q.data(); pb.q_bytes = b.q.size(); pb.t_blob = b.t.data(); pb.t_bytes = b.t.size();
    dagcon_results r;
    const double t0 = wall();
    const int rc = dagcon_consensus_pre(ctx, &pb, &r);
    if (g_timing) fprintf(stderr, "pbdagcon timing: -a batch of %zu records: dagcon_consensus_pre %.3f\n", b.start.size(), wall() - t0);
    if (!ok(ctx, rc, "alignment / consensus")) return 1;
    warn_dropped(ctx, b.start.size());
    return append_results(ctx, b, o, r);
}

// -a --polish N: the alignments come back to the host (the worker's page-locked scratch), round 0's consensus is made from them as
// from .m5 strings, then the rounds.  actx: the context of the first alignment (a local one with --local: the rounds stay global on ctx)
int run_pre_polish(dagcon_ctx *ctx, dagcon_ctx *actx, Batch &b, const Opts &o, Blob *scratch) {
    const double ta0 = wall();
    const size_t A = b.start.size();
    std::vector<uint64_t> ooff(A);
    std::vector<uint32_t> alen(A, 0), nstart(A);
    std::vector<uint32_t> e_qb(A), e_qe(A), e_tb(A), e_te(A);       // the ends of the first alignments
    uint64_t total = 0;
    for (size_t a = 0; a < A; a++) { ooff[a] = total; total += (uint64_t)b.len[a] + b.len2[a]; }
    if (!scratch[0].resize(total + 1, ctx) || !scratch[1].resize(total + 1, ctx)) { fprintf(stderr, "pbdagcon: out of memory\n"); return 1; }
    char *qa = scratch[0].data(), *ta = scratch[1].data();          // the aligned strings
    const double ta1 = wall();
    int rc = dagcon_align(actx, (uint32_t)A, b.off.data(), b.len.data(), b.off2.data(), b.len2.data(), b.q.data(), b.q.size(),
                          b.t.data(), b.t.size(), ooff.data(), &qa[0], &ta[0], alen.data());
    if (rc == DAGCON_OK) rc = dagcon_align_ends(actx, (uint32_t)A, e_qb.data(), e_qe.data(), e_tb.data(), e_te.data());
    if (g_timing) fprintf(stderr, "pbdagcon timing: -a batch of %zu records: buffers %.3f  dagcon_align %.3f\n", A, ta1 - ta0, wall() - ta1);
    if (!ok(actx, rc, "alignment")) return 1;
    warn_dropped(actx, A);
    for (size_t a = 0, g = 0; a < A; a++) {
        while (b.begin[g + 1] <= a) g++;
        // SimpleAligner.cpp:51-62: start = tstart + GenomicTBegin(), end = start + the aligned target span (global:
        // 0 and |tseq|; --local: t_begin and t_end - t_begin, as dagcon_consensus_pre)
        uint32_t start = b.start[a] + (o.local ? e_tb[a] : 0u);
        const uint32_t end = o.local ? b.start[a] + e_te[a] : start + b.len2[a];
        if (b.strand[a] == '-') {
            start = b.tlen[g] - end;
            std::string tmp(alen[a], 0);
            revcomp_into(&tmp[0], &qa[ooff[a]], alen[a]); memcpy(&qa[ooff[a]], tmp.data(), alen[a]);
            revcomp_into(&tmp[0], &ta[ooff[a]], alen[a]); memcpy(&ta[ooff[a]], tmp.data(), alen[a]);
        }
        nstart[a] = start + 1;
    }
    dagcon_batch db = strings_batch(b);
    db.aln_start = nstart.data(); db.aln_off = ooff.data(); db.aln_len = alen.data();
    db.qstr = qa; db.tstr = ta; db.blob_bytes = total;
    dagcon_results r;
    if (!consensus_strings(ctx, db, r)) return 1;
    // --polish: the consensus becomes the backbone, the reads are aligned to it again, N times.  The
    // reference names this use (README.md:14-15) and leaves it to the caller; nothing of it is in its
    // C++ sources, so there is no reference behaviour to match: the steps are this build's own
    // (longest segment as the new backbone, dagcon_align of every read against the stretch of it the
    // read covered before, unaligned target flanks stripped, real-backbone consensus as dazcon.cpp:76).
    // Every round: (1) the longest segment is the new backbone; it covers about positions
    // [trim + range0, trim + range1) of the previous one.  (2) From its previous alignment each read is
    // clipped to what lies over that stretch (plus a margin) and the stretch of the new backbone it covers is
    // estimated; (3) dagcon_align, global over the two pieces, backbone bases in front of / behind the read
    // stripped; (4) real-backbone consensus as dazcon.cpp:76 does.
    const uint32_t T = db.n_targets;
    const uint32_t pad = 64;
    std::vector<uint32_t> cur_start(A), cur_len(A), cur_qbase(A, 0);   // qbase: the read's base the current alignment begins with
    if (o.local)                                     // (the read's first aligned base, in the target's orientation)
        for (size_t a = 0; a < A; a++) cur_qbase[a] = b.strand[a] == '-' ? b.len[a] - e_qe[a] : e_qb[a];
    std::vector<uint64_t> cur_off(A);
    std::string cur_q(qa, db.blob_bytes + 1), cur_t(ta, db.blob_bytes + 1);     // the reads' last alignments, per record
    for (size_t a = 0; a < A; a++) { cur_start[a] = db.aln_start[a]; cur_off[a] = db.aln_off[a]; cur_len[a] = db.aln_len[a]; }
    std::vector<uint64_t> p_qoff(A), p_toff(A), p_ooff(A), p_begin, p_bboff;
    std::vector<uint32_t> p_qlen(A), p_tlen(A), p_alen(A), p_tl, w0(A);
    std::string p_q, p_t, p_qa, p_ta, p_bb, fwd;
    std::vector<uint32_t> k_start, k_len; std::vector<uint64_t> k_off;
    for (unsigned round = 1; round <= o.polish; round++) {
        std::vector<std::string> bb(T);
        std::vector<int32_t> r0(T, 0), r1(T, 0);
        for (uint32_t g = 0; g < T; g++) {
            uint32_t best = 0;                           // (the first of the longest ones, as AlnGraphBoost.cpp:309,319 breaks ties)
            for (uint64_t sg = r.seg_begin[g]; sg < r.seg_begin[g + 1]; sg++)
                if (r.seq_len[sg] > best) { best = r.seq_len[sg]; bb[g].assign(r.seq_blob + r.seq_off[sg], r.seq_len[sg]); r0[g] = r.range0[sg]; r1[g] = r.range1[sg]; }
        }
        p_q.clear(); p_t.clear();
        uint64_t tot = 0;
        size_t g = 0;
        for (size_t a = 0; a < A; a++) {
            while (b.begin[g + 1] <= a) g++;
            const std::string &B = bb[g];
            p_qoff[a] = p_q.size(); p_toff[a] = p_t.size(); p_ooff[a] = tot; p_qlen[a] = 0; p_tlen[a] = 0; w0[a] = 0;
            if (B.empty() || cur_len[a] == 0) { cur_len[a] = 0; continue; }     // (no consensus, or nothing left of the read)
            // the new backbone lies over [lo_t, hi_t) of the previous one, margins included (0-based)
            const int64_t org = (int64_t)o.trim + r0[g];
            const int64_t lo_t = org - pad, hi_t = (int64_t)o.trim + r1[g] + pad;
            int64_t tpos = (int64_t)cur_start[a] - 1;
            uint32_t qpos = 0, qlo = 0, qhi = 0;
            int64_t t_first = -1, t_last = -1;
            for (uint32_t i = 0; i < cur_len[a]; i++) {
                const char qc = cur_q[cur_off[a] + i], tc = cur_t[cur_off[a] + i];
                const bool in = tpos >= lo_t && tpos < hi_t;
                if (qc != '-') { if (tpos < lo_t) qlo = qpos + 1; if (in) qhi = qpos + 1; qpos++; }
                if (in && tc != '-') { if (t_first < 0) t_first = tpos; t_last = tpos; }
                if (tc != '-') tpos++;
            }
            if (qhi <= qlo || t_first < 0) { cur_len[a] = 0; continue; }
            const int64_t a0 = std::max<int64_t>(0, std::min<int64_t>(t_first - org - pad, (int64_t)B.size()));
            const int64_t a1 = std::max<int64_t>(a0, std::min<int64_t>(t_last + 1 - org + pad, (int64_t)B.size()));
            w0[a] = (uint32_t)a0; p_tlen[a] = (uint32_t)(a1 - a0);
            p_t.append(B, (size_t)a0, (size_t)(a1 - a0));
            // the read in the target's orientation, clipped
            fwd.resize(b.len[a]);
            if (b.strand[a] == '-') revcomp_into(&fwd[0], b.q.data() + b.off[a], b.len[a]);
            else memcpy(&fwd[0], b.q.data() + b.off[a], b.len[a]);
            p_qlen[a] = qhi - qlo;
            p_q.append(fwd, cur_qbase[a] + qlo, qhi - qlo);
            cur_qbase[a] += qlo;
            tot += (uint64_t)p_qlen[a] + p_tlen[a];
        }
        p_qa.assign(tot + 1, 0); p_ta.assign(tot + 1, 0);
        if (p_q.empty()) p_q.push_back(0);
        if (p_t.empty()) p_t.push_back(0);
        rc = dagcon_align(ctx, (uint32_t)A, p_qoff.data(), p_qlen.data(), p_toff.data(), p_tlen.data(), p_q.data(), p_q.size(),
                          p_t.data(), p_t.size(), p_ooff.data(), &p_qa[0], &p_ta[0], p_alen.data());
        if (rc != DAGCON_OK) { fprintf(stderr, "pbdagcon: alignment failed (%d): %s\n", rc, dagcon_last_error(ctx)); return 1; }
        // global over the two pieces: backbone bases in front of / behind the read are not part of its alignment
        k_start.clear(); k_off.clear(); k_len.clear();
        p_begin.assign(1, 0);
        g = 0;
        for (size_t a = 0; a < A; a++) {
            while (b.begin[g + 1] <= a) { g++; p_begin.push_back(k_start.size()); }
            if (cur_len[a] == 0) continue;
            uint32_t n = p_alen[a], lead = 0;
            uint64_t off = p_ooff[a];
            while (n && p_qa[off] == '-') { off++; n--; lead++; }
            while (n && p_qa[off + n - 1] == '-') n--;
            cur_start[a] = w0[a] + lead + 1u; cur_off[a] = off; cur_len[a] = n;
            if (n) { k_start.push_back(cur_start[a]); k_off.push_back(off); k_len.push_back(n); }
        }
        while (p_begin.size() < (size_t)T + 1) p_begin.push_back(k_start.size());
        cur_q.swap(p_qa); cur_t.swap(p_ta);            // (the next round clips against these)
        p_tl.assign(T, 0); p_bboff.assign(T, 0); p_bb.clear();
        for (uint32_t t2 = 0; t2 < T; t2++) { p_tl[t2] = (uint32_t)bb[t2].size(); p_bboff[t2] = p_bb.size(); p_bb += bb[t2]; }
        if (p_bb.empty()) p_bb.push_back('N');
        memset(&db, 0, sizeof db);
        db.n_targets = T; db.tlen = p_tl.data(); db.aln_begin = p_begin.data();
        db.aln_start = k_start.data(); db.aln_off = k_off.data(); db.aln_len = k_len.data();
        db.qstr = cur_q.data(); db.tstr = cur_t.data(); db.blob_bytes = cur_q.size();
        db.backbone = p_bb.data(); db.backbone_off = p_bboff.data();
        rc = dagcon_consensus(ctx, &db, &r);
        if (rc != DAGCON_OK) { fprintf(stderr, "pbdagcon: consensus failed (%d): %s\n", rc, dagcon_last_error(ctx)); return 1; }
    }
    return append_results(ctx, b, o, r);
}

int flush(dagcon_ctx *ctx, dagcon_ctx *actx, Batch &b, const Opts &o, Blob *scratch) {
    if (b.ids.empty()) return 0;
    return o.mode == MODE_RECORDS ? run_records(ctx, b, o) : o.mode == MODE_M5 ? run_m5(ctx, b, o)
         : o.polish ? run_pre_polish(ctx, actx, b, o, scratch) : run_pre(ctx, b, o);
}

// ---- consensus workers: one thread + context per GPU and --contexts (the reference starts its N consensus workers itself too,
// main.cpp:251-274); batches are taken in input order from one queue, their records are printed in input order by whoever completes
// the next one in line.  Two contexts per GPU: one batch's copy, host preparation and formatting go on beside the other's kernels ----
struct Workers {
    const Opts &o;
    std::vector<int> dev;                                   // the device of every worker
    std::vector<Batch> bufs;                                // one more than workers: the parser fills one while the others are on GPUs
    std::mutex mu; std::condition_variable cv;
    std::vector<Batch *> free_list, work, done;             // work: FIFO; done: completed, waiting for their turn to print
    unsigned long long next_seq = 0, print_seq = 0;
    bool stop = false; int status = 0;
    dagcon_ctx *pin_ctx = nullptr;                          // first context up: page-locked blobs come from it
    std::vector<std::thread> threads;
    double t_create = 0, t_flush = 0, t_print = 0, t_wait = 0;

    Workers(const Opts &opts, size_t input_bytes) : o(opts) {
        const unsigned per_dev = o.contexts ? o.contexts : (input_bytes > 512ull << 20 ? 2u : 1u);
        for (unsigned k = 0; k < per_dev; k++) for (int d : o.devices) dev.push_back(d);
        bufs = std::vector<Batch>(dev.size() + 1);
        for (auto &x : bufs) free_list.push_back(&x);
    }
    void start() { for (size_t w = 0; w < dev.size(); w++) threads.emplace_back([this, w] { run(w); }); }

    void run(size_t w) {
        dagcon_ctx *ctx = nullptr;
        const double tc0 = wall();
        int rc = dg_create(o.min_cov, o.min_len, o.trim, dev[w], (o.local && !o.polish ? DAGCON_FLAG_LOCAL_ALIGN : 0u) | (o.fastq ? DAGCON_FLAG_BASE_SUPPORT : 0u) | (o.want_edits() ? DAGCON_FLAG_BASE_POS : 0u), &o.pick, &ctx);
        if (rc == DAGCON_OK && o.want_edits() && ((rc = dagcon_set_edits(ctx, 1)) != DAGCON_OK || (o.want_edit_support() && (rc = dagcon_set_edit_support(ctx, 1)) != DAGCON_OK) ||
                                                   (!o.hap.vcf.empty() && (rc = dagcon_set_hap_calls(ctx, 1)) != DAGCON_OK))) {
            fprintf(stderr, "pbdagcon: %s\n", dagcon_last_error(ctx));
            dagcon_destroy(ctx); ctx = nullptr;
        }
        if (rc == DAGCON_OK && o.want_pile()) {
            const dagcon_pileup_opts po = {o.pile.min_count, o.pile.min_frac_ppm};
            if ((rc = dagcon_set_pileup(ctx, &po)) != DAGCON_OK) { fprintf(stderr, "pbdagcon: %s\n", dagcon_last_error(ctx)); dagcon_destroy(ctx); ctx = nullptr; }
        }
        if (rc == DAGCON_OK && o.want_sr()) {
            const dagcon_site_reads_opts so = {o.want_phase() ? 1u : 0u, 0u};
            if ((rc = dagcon_set_site_reads(ctx, &so)) != DAGCON_OK) { fprintf(stderr, "pbdagcon: %s\n", dagcon_last_error(ctx)); dagcon_destroy(ctx); ctx = nullptr; }
        }
        if (rc == DAGCON_OK && o.want_al() && (rc = dagcon_set_site_alleles(ctx, 1)) != DAGCON_OK) { fprintf(stderr, "pbdagcon: %s\n", dagcon_last_error(ctx)); dagcon_destroy(ctx); ctx = nullptr; }
        if (rc == DAGCON_OK && o.jn.on() && (rc = dagcon_set_site_join(ctx, 1)) != DAGCON_OK) { fprintf(stderr, "pbdagcon: %s\n", dagcon_last_error(ctx)); dagcon_destroy(ctx); ctx = nullptr; }
        if (rc == DAGCON_OK && o.link.on && (rc = dagcon_set_site_link(ctx, &o.link.o)) != DAGCON_OK) { fprintf(stderr, "pbdagcon: %s\n", dagcon_last_error(ctx)); dagcon_destroy(ctx); ctx = nullptr; }
        if (rc == DAGCON_OK && o.hap.on()) {
            const dagcon_hap_opts ho = {o.hap.min_sites, o.hap.min_reads};
            if ((rc = dagcon_set_hap_consensus(ctx, &ho)) != DAGCON_OK) { fprintf(stderr, "pbdagcon: %s\n", dagcon_last_error(ctx)); dagcon_destroy(ctx); ctx = nullptr; }
        }
        dagcon_ctx *actx = ctx;                             // --local --polish: the first alignment on a local context of its own
        if (rc == DAGCON_OK && o.local && o.polish) {       // (aligns only: the support comes from ctx's last round)
            rc = dg_create(o.min_cov, o.min_len, o.trim, dev[w], DAGCON_FLAG_LOCAL_ALIGN, nullptr, &actx);
            if (rc != DAGCON_OK) { dagcon_destroy(ctx); ctx = nullptr; }
        }
        if (w == 0) t_create = wall() - tc0;
        if (rc != DAGCON_OK) {
            std::lock_guard<std::mutex> lk(mu);
            status = 1;
            cv.notify_all();
            return;
        }
        { std::lock_guard<std::mutex> lk(mu); if (!pin_ctx) pin_ctx = ctx; }
        Blob scratch[2];
        for (;;) {
            Batch *b = nullptr;
            {
                std::unique_lock<std::mutex> lk(mu);
                cv.wait(lk, [&] { return !work.empty() || stop; });
                if (work.empty()) break;
                b = work.front(); work.erase(work.begin());
            }
            const double tf0 = wall();
            const int st = flush(ctx, actx, *b, o, scratch);
            const double tf = wall() - tf0;
            {
                std::unique_lock<std::mutex> lk(mu);
                t_flush += tf;
                if (st) status = st;
                done.push_back(b);
                // print what is next in line (this batch and any that were waiting on it)
                for (size_t i = 0; i < done.size();) {
                    if (done[i]->seq != print_seq) { i++; continue; }
                    Batch *d = done[i];
                    done.erase(done.begin() + i);
                    { const double tp0 = wall(); fwrite(d->out.data(), 1, d->out.size(), stdout); t_print += wall() - tp0; }
                    if (g_edits) { fwrite(d->edits.data(), 1, d->edits.size(), g_edits); g_n_edits += d->n_edits; }
                    if (g_vcf) { g_vcf_contigs += d->contigs; if (fwrite(d->vcf.data(), 1, d->vcf.size(), g_vcf_lines) != d->vcf.size()) g_vcf_bad = true; }
                    if (g_pileup && fwrite(d->pileup.data(), 1, d->pileup.size(), g_pileup) != d->pileup.size()) g_pile_bad = true;
                    if (g_sites && fwrite(d->sites.data(), 1, d->sites.size(), g_sites) != d->sites.size()) g_pile_bad = true;
                    if (g_site_reads && fwrite(d->site_reads.data(), 1, d->site_reads.size(), g_site_reads) != d->site_reads.size()) g_pile_bad = true;
                    if (g_haplotag && fwrite(d->haplotag.data(), 1, d->haplotag.size(), g_haplotag) != d->haplotag.size()) g_pile_bad = true;
                    if (g_hap_out && fwrite(d->hap_out.data(), 1, d->hap_out.size(), g_hap_out) != d->hap_out.size()) g_pile_bad = true;
                    if (g_hap_sites && fwrite(d->hap_sites.data(), 1, d->hap_sites.size(), g_hap_sites) != d->hap_sites.size()) g_pile_bad = true;
                    if (g_linked_sites && fwrite(d->linked_sites.data(), 1, d->linked_sites.size(), g_linked_sites) != d->linked_sites.size()) g_pile_bad = true;
                    if (g_hap_vcf) { g_hap_vcf_contigs += d->hap_contigs; if (fwrite(d->hap_vcf.data(), 1, d->hap_vcf.size(), g_hap_vcf_lines) != d->hap_vcf.size()) g_pile_bad = true; }
                    if (g_site_alleles && fwrite(d->site_alleles.data(), 1, d->site_alleles.size(), g_site_alleles) != d->site_alleles.size()) g_pile_bad = true;
                    if (g_site_vcf) { g_site_vcf_contigs += d->site_contigs; if (fwrite(d->site_vcf.data(), 1, d->site_vcf.size(), g_site_vcf_lines) != d->site_vcf.size()) g_pile_bad = true; }
                    if (g_joined_alleles && fwrite(d->joined_alleles.data(), 1, d->joined_alleles.size(), g_joined_alleles) != d->joined_alleles.size()) g_pile_bad = true;
                    if (g_joined_vcf) { g_joined_vcf_contigs += d->joined_contigs; if (fwrite(d->joined_vcf.data(), 1, d->joined_vcf.size(), g_joined_vcf_lines) != d->joined_vcf.size()) g_pile_bad = true; }
                    d->clear();
                    free_list.push_back(d);
                    print_seq++;
                    i = 0;
                }
            }
            cv.notify_all();
        }
        // (blobs that were page-locked through this context are released before it goes)
        {
            std::unique_lock<std::mutex> lk(mu);
            for (auto &x : bufs) { if (x.q.owner == ctx) x.q.release(); if (x.t.owner == ctx) x.t.release(); }
            if (pin_ctx == ctx) pin_ctx = nullptr;
        }
        scratch[0].release(); scratch[1].release();
        if (actx != ctx) dagcon_destroy(actx);
        dagcon_destroy(ctx);
    }
    dagcon_ctx *pin() { std::lock_guard<std::mutex> lk(mu); return pin_ctx; }
    // a free batch buffer for the parser (waits for a worker to finish one); NULL: a worker gave up
    Batch *acquire() {
        std::unique_lock<std::mutex> lk(mu);
        cv.wait(lk, [&] { return !free_list.empty() || status; });
        if (free_list.empty()) return nullptr;
        Batch *b = free_list.back(); free_list.pop_back();
        return b;
    }
    // hands the filled batch to the workers and takes the next free buffer; the status so far
    int submit(Batch *&b) {
        {
            std::lock_guard<std::mutex> lk(mu);
            if (status) return status;
            b->seq = next_seq++;
            work.push_back(b);
        }
        cv.notify_all();
        const double tw0 = wall();
        b = acquire();
        t_wait += wall() - tw0;
        return b ? 0 : 1;
    }
    // every submitted batch printed (or a worker gave up), every worker gone: each destroys its context, so the device
    // memory goes back in order and the next process's large hipMalloc does not wait for it
    int drain() {
        {
            std::unique_lock<std::mutex> lk(mu);
            cv.wait(lk, [&] { return print_seq == next_seq || status; });
            stop = true;
        }
        cv.notify_all();
        for (auto &w : threads) w.join();
        return status;
    }
};

// ---- the input ---------------------------------------------------------------------------------------------------------
struct Input {
    const char *data = nullptr; size_t size = 0;
    std::string slurp;                 // stdin
    void *map = nullptr;               // a file
    size_t unmapped = 0;               // pages of map dropped so far
    unsigned nthr = 1;                 // host threads of every stage (-j)

    // mmap a file, or slurp stdin
    bool open(const std::string &path) {
        if (path == "-") {
            char buf[1 << 16];
            size_t n;
            while ((n = fread(buf, 1, sizeof buf, stdin)) > 0) slurp.append(buf, n);
            data = slurp.data(); size = slurp.size();
            return true;
        }
        int fd = ::open(path.c_str(), O_RDONLY);
        if (fd < 0) { fprintf(stderr, "pbdagcon: error opening file: %s\n", path.c_str()); return false; }
        struct stat st;
        if (fstat(fd, &st) != 0) { close(fd); return false; }
        size = (size_t)st.st_size;
        if (size) {
            map = mmap(nullptr, size, PROT_READ, MAP_PRIVATE, fd, 0);
            if (map == MAP_FAILED) { fprintf(stderr, "pbdagcon: mmap failed\n"); close(fd); return false; }
            data = (const char *)map;
        }
        close(fd);
        return true;
    }
    // the text is finished with (--bam: the inflated records take its place)
    void replace(const char *d, size_t n) {
        if (map) { munmap(map, size); map = nullptr; }
        slurp.clear(); slurp.shrink_to_fit();
        data = d; size = n;
    }
    // where the line that holds byte p ends (p itself at the end of the input)
    size_t line_end(size_t p) const {
        if (p >= size) return size;
        const char *nl = (const char *)memchr(data + p, '\n', size - p);
        return nl ? (size_t)(nl - data) + 1 : size;
    }
    // The text in front of `dead` is finished with: its page-table entries go now, while the GPU works, instead of all at once at
    // the end (0.3 s for 26 GB of text).  MADV_DONTNEED takes the address-space lock shared (munmap takes it exclusively and would
    // stall the workers' page faults and the driver's pinning): the threads drop a share of the range each
    void drop_pages(size_t dead) {
        const size_t upto = dead & ~(size_t)((2u << 20) - 1);
        if (!map || upto <= unmapped) return;
        const size_t n2m = (upto - unmapped) >> 21;
        on_threads(nthr, [&](unsigned k) {
            const size_t a = unmapped + ((n2m * k / nthr) << 21), e = unmapped + ((n2m * (k + 1) / nthr) << 21);
            if (e > a) madvise((char *)map + a, e - a, MADV_DONTNEED);
        });
        unmapped = upto;
    }
};

// ---- parse (Alignment.cpp:44-80) and group by target id (BlasrM5AlnProvider.cpp:34-55) ----
// 1. index: the -j threads split the text at line starts and record where every field of every record is (nothing is
//    copied);
// 2. in file order: records are grouped into targets and targets into batches;
// 3. per batch the same threads copy (or reverse-complement) the strings into the blobs.
// The text is taken a slab at a time, so that the first batch reaches the GPU before the whole file has been indexed;
// the records of a slab's last (possibly unfinished) target are carried into the next slab.

// what one thread found in its piece of a slab
template <class R>
struct Part { std::vector<R> recs; int err = 0; unsigned long long err_rec = 0; int err_nf = 0; unsigned long long lines = 0, skipped = 0, no_md = 0; };

// what the two indexers share: the slab's records in file order (the carried ones first), up to the first malformed one
template <class R>
struct Indexer {
    Input &in;
    std::vector<R> carry;
    std::vector<Part<R>> parts;
    std::vector<const R *> recs;
    bool had_error = false;
    unsigned long long n_rec_before = 0;
    double t_index = 0, t_fill = 0;                        // PBDAGCON_TIMING
    explicit Indexer(Input &i) : in(i), parts(i.nthr) {}
    void begin() { recs.clear(); for (const R &r : carry) recs.push_back(&r); }
    void take(const Part<R> &p) { for (const R &r : p.recs) recs.push_back(&r); n_rec_before += p.recs.size(); }
    // [s0, s1) cut at line starts into a piece per thread; thread k has line(part k, text, length) parse every line of
    // its piece, until it returns false
    template <class Line>
    void index_lines(size_t s0, size_t s1, Line line) {
        const unsigned nthr = in.nthr;
        std::vector<size_t> cut(nthr + 1, s1);
        cut[0] = s0;
        for (unsigned k = 1; k < nthr; k++) {
            size_t p0 = std::max(cut[k - 1], s0 + (size_t)((unsigned long long)(s1 - s0) * k / nthr));
            if (p0 > s0 && p0 < s1) p0 = std::min(in.line_end(p0 - 1), s1);
            cut[k] = std::min(p0, s1);
        }
        on_threads(nthr, [&](unsigned k) {
            Part<R> &pt = parts[k];
            pt.recs.clear(); pt.err = 0; pt.lines = 0; pt.skipped = 0; pt.no_md = 0;
            for (size_t pos = cut[k]; pos < cut[k + 1];) {
                const char *text = in.data + pos;
                const size_t ll = dg_line(in.data, in.size, pos);
                pt.lines++;
                if (!line(pt, text, ll)) return;
            }
        });
    }
};

// a record of .m5 or .pre text
struct Rec {
    const char *rname, *qname, *q, *t;                     // target and query name, as DgAlnRec calls them
    uint32_t rname_len, qname_len, len, tl, tlen, start;   // len, tl: of the query and the target string; tlen: of the target
    char strand;
};

struct TextIndexer : Indexer<Rec> {
    const Opts &o;
    TextIndexer(Input &i, const Opts &opts) : Indexer<Rec>(i), o(opts) {}

    static bool parse_line(Mode mode, Part<Rec> &pt, const char *line, size_t ll) {
        const char *f[19];
        size_t fl[19], i = 0;
        int nf = 0;
        while (i < ll && nf < 19) {
            while (i < ll && line[i] == ' ') i++;
            if (i >= ll) break;
            const char *sp = (const char *)memchr(line + i, ' ', ll - i);   // fields 16..18 are ~tlen chars each
            const size_t j = sp ? (size_t)(sp - line) : ll;
            f[nf] = line + i; fl[nf] = j - i; nf++;
            i = j;
        }
        if (nf == 0) return true;                       // blank line
        Rec r;
        if (mode == MODE_PRE) {
            // Alignment.cpp:82-112 parsePre: qid tid strand tlen tstart tend qseq tseq
            if (nf < 8) { pt.err = 1; pt.err_rec = pt.recs.size() + 1; pt.err_nf = nf; return false; }
            r.rname = f[1]; r.rname_len = (uint32_t)fl[1];
            r.qname = f[0]; r.qname_len = (uint32_t)fl[0];
            r.strand = f[2][0];
            r.tlen = tok_u32(f[3], fl[3]);
            r.start = tok_u32(f[4], fl[4]);             // (SimpleAligner.cpp:61 adds the 1)
            r.q = f[6]; r.len = (uint32_t)fl[6];
            r.t = f[7]; r.tl = (uint32_t)fl[7];
        } else {
            if (nf < 19) { pt.err = 1; pt.err_rec = pt.recs.size() + 1; pt.err_nf = nf; return false; }
            if (fl[16] != fl[18]) { pt.err = 2; pt.err_rec = pt.recs.size() + 1; return false; }
            r.rname = f[5]; r.rname_len = (uint32_t)fl[5];
            r.qname = f[0]; r.qname_len = (uint32_t)fl[0];
            r.q = f[16]; r.t = f[18]; r.len = (uint32_t)fl[16]; r.tl = r.len;
            r.tlen = tok_u32(f[6], fl[6]);
            r.start = tok_u32(f[7], fl[7]) + 1;             // Alignment.cpp:65-66
            r.strand = f[9][0];
        }
        pt.recs.push_back(r);
        return true;
    }
    // indexes the slab that begins at s0; where the next one begins
    size_t index(size_t s0, size_t slab_bytes) {
        const size_t s1 = in.line_end(std::min(in.size, s0 + slab_bytes));   // a slab ends at a line end
        index_lines(s0, s1, [this](Part<Rec> &pt, const char *text, size_t ll) { return parse_line(o.mode, pt, text, ll); });
        begin();
        for (const Part<Rec> &pt : parts) {
            take(pt);
            if (pt.err == 1) fprintf(stderr, "pbdagcon: format error: record %llu has %d fields, %d expected\n", n_rec_before + 1, pt.err_nf, o.mode == MODE_PRE ? 8 : 19);
            if (pt.err == 2) fprintf(stderr, "pbdagcon: format error: record %llu: query and target strings differ in length\n", n_rec_before + 1);
            if (pt.err) { had_error = true; break; }
        }
        return s1;
    }
    bool add_target(Batch &b, const Rec &r, size_t &) { b.ids.emplace_back(r.rname, r.rname_len); b.tlen.push_back(r.tlen); return true; }
    void add_record(Batch &b, const Rec &r, size_t &bytes, size_t &bytes2) {
        b.start.push_back(r.start); b.len.push_back(r.len); b.len2.push_back(r.tl);
        b.off.push_back(bytes); b.off2.push_back(bytes2);
        b.strand.push_back(r.strand);
        if (o.sr.on()) b.qnames.emplace_back(r.qname, r.qname_len);
        bytes += r.len; bytes2 += r.tl;                     // (-a: the t strings count too)
    }
    // copies the strings of records [r0, r1) into batch b, whose offsets are set already
    void fill(Batch &b, size_t r0, size_t r1) {
        on_threads(in.nthr, [&](unsigned k) {
            for (size_t x = r0 + k; x < r1; x += in.nthr) {
                const Rec &r = *recs[x];
                char *dq = b.q.data() + b.off[x - r0], *dt = b.t.data() + b.off2[x - r0];
                if (o.mode == MODE_M5 && r.strand == '-') {     // Alignment.cpp:69-75: start is NOT flipped (Q6)
                    revcomp_into(dq, r.q, r.len);
                    revcomp_into(dt, r.t, r.len);
                } else {                                        // (.pre: sequences as they are, Alignment.cpp:112)
                    memcpy(dq, r.q, r.len);
                    memcpy(dt, r.t, r.tl);
                }
            }
        });
    }
    // --dump-parsed: the batch as it would go to the device
    void dump(Batch &b, size_t r0, size_t r1) {
        for (size_t y = r0, g = 0; y < r1; y++) {
            const Rec &r = *recs[y];
            while (b.begin[g + 1] <= y - r0) g++;
            printf("%.*s\t%u\t%u\t%c\t%.*s\t%.*s\t%.*s\n", (int)r.rname_len, r.rname, b.tlen[g], r.start, r.strand,
                   (int)r.qname_len, r.qname, (int)r.len, b.q.data() + b.off[y - r0], (int)r.tl, b.t.data() + b.off2[y - r0]);
        }
    }
    void report_skipped() {}
};

// records of a DgRecordKind: --sam text is indexed like .m5 text, on the -j threads; --bam by one thread that stops at
// the slab's end (there is no per-base work in it); --paf all at once (paf.h has parsed, checked and grouped the lines)
struct RecordIndexer : Indexer<DgAlnRec> {
    const Opts &o; const DgKindDesc &kd; const DgRefSeqs &ref;
    DgBamReader &bam;
    const DgPafInput &paf;
    unsigned long long n_lines_before = 0, n_skipped = 0, n_no_md = 0;
    std::unordered_set<std::string> seen_targets;         // a target whose records come back after another's is an error

    RecordIndexer(Input &i, const Opts &opts, const DgRefSeqs &rf, DgBamReader &bm, const DgPafInput &pf)
        : Indexer<DgAlnRec>(i), o(opts), kd(dg_kind(opts.kind)), ref(rf), bam(bm), paf(pf) {}

    size_t index(size_t s0, size_t slab_bytes) {
        if (dg_kind_sam(o.kind)) return index_sam(s0, in.line_end(std::min(in.size, s0 + slab_bytes)));
        begin();
        Part<DgAlnRec> &pt = parts[0];
        pt.recs.clear();
        if (dg_kind_bam(o.kind)) {
            const size_t s1 = std::min(in.size, s0 + slab_bytes);
            DgBamRec br; DgAlnRec r; std::string err;
            while (bam.at < s1) {                          // (the reader stops behind the first record that ends at s1 or later)
                const int rc = bam.next(br, err);
                if (rc == 0) break;
                if (rc < 0) { fprintf(stderr, "pbdagcon: format error: %s\n", err.c_str()); had_error = true; break; }
                dg_bam_rec(bam, br, ref, r, dg_kind_md(o.kind));
                if (!r.target) { fprintf(stderr, "pbdagcon: record %llu: RNAME is not a sequence of %s\n", br.ordinal, o.ref.c_str()); had_error = true; break; }
                if (dg_kind_md(o.kind) && !r.md) { n_no_md++; continue; }
                pt.recs.push_back(r);
            }
            n_skipped = bam.n_skipped;
            take(pt);
            return bam.at >= in.size ? in.size : std::max(bam.at, s0);   // behind the last record taken
        }
        pt.recs.resize(paf.recs.size());
        for (size_t k = 0; k < paf.recs.size(); k++) dg_paf_rec(paf.recs[k], o.kind == DG_REC_CS, pt.recs[k]);
        n_skipped = paf.n_secondary;
        take(pt);
        return in.size;
    }
    // QNAME FLAG RNAME POS MAPQ CIGAR RNEXT PNEXT TLEN SEQ QUAL, tab-separated; header lines skipped
    size_t index_sam(size_t s0, size_t s1) {
        index_lines(s0, s1, [this](Part<DgAlnRec> &pt, const char *text, size_t ll) {
            DgSamLine sm;
            const DgSamWhat what = dg_sam_split(text, ll, sm, tok_u32);
            if (what == DG_SAM_NO_RECORD) return true;
            if (what == DG_SAM_SKIPPED) { pt.skipped++; return true; }
            pt.err_rec = pt.lines;
            if (what == DG_SAM_FEW_FIELDS) { pt.err = 1; pt.err_nf = sm.nf; return false; }
            if (what == DG_SAM_BAD_CIGAR) { pt.err = 3; return false; }
            DgAlnRec r;
            dg_sam_rec(sm, tok_u32(sm.f[3], sm.fl[3]), pt.lines, ref, r, dg_kind_md(o.kind));
            if (!r.target) { pt.err = 4; return false; }
            if (dg_kind_md(o.kind) && !r.md) { pt.no_md++; return true; }
            pt.recs.push_back(r);
            return true;
        });
        begin();
        for (Part<DgAlnRec> &pt : parts) {
            for (DgAlnRec &r : pt.recs) r.where += n_lines_before;      // line numbers of the whole input
            n_skipped += pt.skipped; n_no_md += pt.no_md;
            take(pt);
            if (pt.err) {
                const unsigned long long ln = n_lines_before + pt.err_rec;
                if (pt.err == 1) fprintf(stderr, "pbdagcon: format error: line %llu has %d fields, 11 expected\n", ln, pt.err_nf);
                else if (pt.err == 3) fprintf(stderr, "pbdagcon: format error: line %llu: malformed CIGAR\n", ln);
                else if (dg_kind_md(o.kind)) fprintf(stderr, "pbdagcon: line %llu: RNAME has no @SQ line in the header (--md takes the targets' names and lengths from there)\n", ln);
                else fprintf(stderr, "pbdagcon: line %llu: RNAME is not a sequence of %s\n", ln, o.ref.c_str());
                had_error = true; break;
            }
            n_lines_before += pt.lines;
        }
        return s1;
    }
    bool add_target(Batch &b, const DgAlnRec &r, size_t &bytes2) {
        if (!seen_targets.emplace(r.rname, r.rname_len).second) {
            fprintf(stderr, "pbdagcon: %s %llu: records of %.*s come back after another target's; the records of one RNAME "
                    "must be consecutive (sort the %s by coordinate)\n", kd.unit, r.where, (int)r.rname_len, r.rname, kd.format);
            return false;
        }
        b.ids.emplace_back(r.rname, r.rname_len);
        b.tlen.push_back(r.target->len);
        b.toff.push_back(bytes2); b.tsrc.push_back(dg_kind_md(o.kind) ? nullptr : ref.bases.data() + r.target->off); bytes2 += r.target->len;
        return true;
    }
    void add_record(Batch &b, const DgAlnRec &r, size_t &bytes, size_t &) {
        b.opb.push_back(b.opb.back() + r.nops);
        b.start.push_back(r.pos);
        b.off.push_back(bytes); b.len.push_back(r.q_len);
        b.reverse.push_back(r.reverse ? 1 : 0);
        if (o.sr.on()) b.qnames.emplace_back(r.qname, r.qname_len);
        if (o.kind == DG_REC_CS) { b.cs_len.push_back(r.cs_len); b.tspan.push_back(r.t_span); }
        if (dg_kind_md(o.kind)) { b.md_off.push_back(b.md.size()); b.md_len.push_back(r.md_len); b.md.append(r.md, r.md_len); }
        bytes += dg_blob_bytes(o.kind, r);
    }
    // the targets' bases, once each; of every record its bytes of the q blob as they lie in the input and its ops
    void fill(Batch &b, size_t r0, size_t r1) {
        b.ops.resize(b.opb.back());
        on_threads(in.nthr, [&](unsigned k) {
            for (size_t g = k; g < b.tsrc.size(); g += in.nthr) if (b.tsrc[g]) memcpy(b.t.data() + b.toff[g], b.tsrc[g], b.tlen[g]);
            for (size_t x = r0 + k; x < r1; x += in.nthr) {
                const DgAlnRec &r = *recs[x];
                memcpy(b.q.data() + b.off[x - r0], dg_blob(o.kind, r), dg_blob_bytes(o.kind, r));
                dg_rec_ops(o.kind, r, b.ops.data() + b.opb[x - r0]);
            }
        });
    }
    // --dump-parsed: what --sam prints for the SAM record of the same alignment -- RNAME, its length in --ref, POS, strand, QNAME,
    // SEQ, CIGAR (from the batch's ops) -- with SEQ and CIGAR made for printing only where the kind has neither: --bam: SEQ decoded;
    // --paf: SEQ the whole read in the target's orientation, soft clips qs and qlen - qe around the cg ops, swapped for '-'; --cs:
    // SEQ the decoded read, the CIGAR the decoded = X I D ops
    void dump(Batch &b, size_t r0, size_t r1) {
        for (size_t y = r0; y < r1; y++) {
            const DgAlnRec &r = *recs[y];
            const char *q = b.q.data() + b.off[y - r0];
            std::string seq(q, dg_kind_sam(o.kind) ? r.q_len : 0);
            std::string cigar = dg_cigar_text(b.ops.data() + b.opb[y - r0], b.opb[y - r0 + 1] - b.opb[y - r0]);
            if (dg_kind_bam(o.kind)) {
                for (uint32_t i = 0; i < r.q_len; i++) seq += dg_bam_base((const uint8_t *)q, i);
            } else if (o.kind == DG_REC_STRANDED) {
                const uint32_t c0 = r.reverse ? r.read_len - r.qs - r.q_len : r.qs, c1 = r.read_len - r.q_len - c0;
                seq = r.reverse ? dg_paf_revcomp(r.read, r.read_len) : std::string(r.read, r.read_len);
                cigar = (c0 ? std::to_string(c0) + "S" : "") + cigar + (c1 ? std::to_string(c1) + "S" : "");
            } else if (o.kind == DG_REC_CS) {
                std::vector<uint32_t> dops;
                if (!dg_cs_decode(q, r.cs_len, ref.bases.data() + r.target->off, r.target->len, r.pos, seq, dops)) { seq = "*"; dops.clear(); }
                cigar = dg_cigar_text(dops.data(), dops.size());
            }
            printf("%.*s\t%u\t%u\t%c\t%.*s\t%s\t%s", (int)r.rname_len, r.rname, r.target->len, r.pos, r.reverse ? '-' : '+',
                   (int)r.qname_len, r.qname, seq.c_str(), cigar.c_str());
            if (dg_kind_md(o.kind)) printf("\t%.*s", (int)b.md_len[y - r0], b.md.data() + b.md_off[y - r0]);   // (the text as the batch carries it)
            putchar('\n');
        }
    }
    void report_skipped() {
        if (o.verbose) fprintf(stderr, "pbdagcon: %llu %s\n", n_skipped, kd.skipped_what);
        dg_report_no_md(o.kind, n_no_md);
    }
};

// per slab: index -> group into batches -> fill -> submit (or dump); the status
template <class Ix>
int parse_input(Ix &ix, size_t first, const Opts &o, Workers &wk) {
    Input &in = ix.in;
    const size_t slab_bytes = o.slab_bytes ? o.slab_bytes : std::max<size_t>(o.batch_bytes, 256u << 20);
    const bool want_pin = o.pinned == 1 || (o.pinned < 0 && in.size > 2 * o.batch_bytes);
    auto same_target = [](const auto &x, const auto &y) { return x.rname_len == y.rname_len && memcmp(x.rname, y.rname, x.rname_len) == 0; };
    int status = 0;
    Batch *b = o.dump ? &wk.bufs[0] : wk.acquire();
    if (!b) status = 1;
    size_t slab_pos = first;
    while (status == 0 && !ix.had_error && (slab_pos < in.size || !ix.carry.empty())) {
        { const double t0 = wall(); slab_pos = ix.index(slab_pos, slab_bytes); ix.t_index += wall() - t0; }
        const auto &recs = ix.recs;
        const bool eof = slab_pos >= in.size || ix.had_error;
        // all but the last target of the slab (it may go on in the next one)
        size_t n_use = recs.size();
        if (!eof) while (n_use > 0 && same_target(*recs[n_use - 1], *recs.back())) n_use--;
        size_t rb = 0, bytes = 0, bytes2 = 0;            // first record of the batch being formed; bytes of its q and t blobs
        for (size_t x = 0; x <= n_use && status == 0; x++) {
            const bool last = x == n_use;
            const bool new_target = !last && (x == rb || !same_target(*recs[x], *recs[x - 1]));
            // a batch is closed when it is full, and at the end of the slab's usable records once it
            // holds something (at the end of the input whatever it holds)
            if (last || (new_target && x > rb && (b->ids.size() >= o.batch_targets || bytes + bytes2 >= o.batch_bytes))) {
                if (x > rb) {
                    b->begin.push_back(b->start.size());
                    const double t0 = wall();
                    dagcon_ctx *pin = want_pin ? wk.pin() : nullptr;
                    if (!b->q.resize(bytes, pin) || !b->t.resize(bytes2, pin)) { fprintf(stderr, "pbdagcon: out of memory\n"); exit(1); }
                    ix.fill(*b, rb, x);
                    ix.t_fill += wall() - t0;
                    if (o.dump) { ix.dump(*b, rb, x); b->clear(); }
                    else status = wk.submit(b);
                }
                rb = x; bytes = 0; bytes2 = 0;
                if (last || status) break;
            }
            if (new_target) {
                if (x > rb) b->begin.push_back(b->start.size());
                if (!ix.add_target(*b, *recs[x], bytes2)) { ix.had_error = true; break; }
            }
            ix.add_record(*b, *recs[x], bytes, bytes2);
        }
        // the unfinished target's records wait for the next slab
        decltype(ix.carry) next_carry;
        for (size_t x = n_use; x < recs.size(); x++) next_carry.push_back(*recs[x]);
        ix.carry.swap(next_carry);
        // the text in front of the first carried record is finished with
        in.drop_pages(ix.carry.empty() ? slab_pos : (size_t)(ix.carry[0].qname - in.data));    // (a line begins with its query name)
        if (eof && ix.carry.empty()) break;
        if (eof) slab_pos = in.size;
    }
    ix.report_skipped();
    return ix.had_error ? 1 : status;
}

}  // namespace

int main(int argc, char **argv) {
    Opts o;
    if (int rc = parse_args(argc, argv, o)) return rc;
    if (o.dump && o.pick.on()) fprintf(stderr, "pbdagcon: record filter: max_error_ppm %u max_depth %u\n", o.pick.max_error_ppm, o.pick.max_depth);
    g_timing = getenv("PBDAGCON_TIMING") != nullptr;
    const double t_main = wall();
    Input in;
    in.nthr = std::max(1u, std::min(o.threads, 64u));
    if (!in.open(o.input)) return 1;
    // ---- records: the targets' bases (--sam: and the header's @SQ lines against them); --bam: the file inflated (the -j threads), its
    // header's references against --ref, from here on the input is the inflated records; --paf: the reads, and every line parsed,
    // checked and grouped by target (targets in --ref order) ----
    DgRefSeqs ref; DgBamReader bam; DgPafInput paf;
    size_t first = 0;                                      // where the first record lies
    if (o.mode == MODE_RECORDS) {
        std::string err;
        bool good = dg_kind_md(o.kind) || dg_read_fasta(o.ref, ref, err);
        if (good && o.kind == DG_REC_PLAIN) good = dg_sam_check_header(in.data, in.size, ref, err);
        if (good && o.kind == DG_REC_PLAIN_MD) good = dg_sam_header_refs(in.data, in.size, ref, err);
        if (good && dg_kind_bam(o.kind)) good = bam.open((const uint8_t *)in.data, in.size, o.threads, err);
        if (good && o.kind == DG_REC_PACKED) good = dg_bam_check_refs(bam, ref, err);
        if (good && o.kind == DG_REC_PACKED_MD) good = dg_bam_header_refs(bam, ref, err);
        paf.cs = o.kind == DG_REC_CS;
        if (good && o.kind == DG_REC_STRANDED) good = dg_read_reads(o.reads, paf.reads, err);
        if (good && (o.kind == DG_REC_STRANDED || o.kind == DG_REC_CS)) good = paf.parse(in.data, in.size, ref, err);
        if (!good) { fprintf(stderr, "pbdagcon: %s\n", err.c_str()); return 1; }
    }
    if (o.mode == MODE_RECORDS && dg_kind_bam(o.kind)) {
        const DgBgzfStats &bs = bam.stats;
        if (o.verbose && !bs.eof_member) fprintf(stderr, "pbdagcon: note: the BAM file does not end with the empty BGZF member (it may be incomplete)\n");
        if (g_timing)
            fprintf(stderr, "pbdagcon timing: --bam inflate: %zu members, %.1f MB -> %.1f MB in %.3f on %u threads (%.1f MB/s of inflated bytes per thread)\n",
                    bs.members, bs.file_bytes / 1e6, bs.inflated_bytes / 1e6, bs.wall, bs.threads, bs.busy > 0 ? bs.inflated_bytes / 1e6 / bs.busy : 0.0);
        in.replace((const char *)bam.u.data(), bam.u.size());
        first = bam.at;
    }

    // ---- --pileup / --sites: both files are opened before anything runs ----
    if (!o.pile.pileup.empty() && !(g_pileup = fopen(o.pile.pileup.c_str(), "w"))) { fprintf(stderr, "pbdagcon: cannot write %s\n", o.pile.pileup.c_str()); return 1; }
    if (!o.pile.sites.empty() && !(g_sites = fopen(o.pile.sites.c_str(), "w"))) { fprintf(stderr, "pbdagcon: cannot write %s\n", o.pile.sites.c_str()); return 1; }
    if (!o.sr.site_reads.empty() && !(g_site_reads = fopen(o.sr.site_reads.c_str(), "w"))) { fprintf(stderr, "pbdagcon: cannot write %s\n", o.sr.site_reads.c_str()); return 1; }
    if (!o.sr.haplotag.empty() && !(g_haplotag = fopen(o.sr.haplotag.c_str(), "w"))) { fprintf(stderr, "pbdagcon: cannot write %s\n", o.sr.haplotag.c_str()); return 1; }
    if (!o.hap.consensus.empty() && !(g_hap_out = fopen(o.hap.consensus.c_str(), "w"))) { fprintf(stderr, "pbdagcon: cannot write %s\n", o.hap.consensus.c_str()); return 1; }
    if (!o.hap.sites.empty() && !(g_hap_sites = fopen(o.hap.sites.c_str(), "w"))) { fprintf(stderr, "pbdagcon: cannot write %s\n", o.hap.sites.c_str()); return 1; }
    if (!o.link.linked.empty() && !(g_linked_sites = fopen(o.link.linked.c_str(), "w"))) { fprintf(stderr, "pbdagcon: cannot write %s\n", o.link.linked.c_str()); return 1; }
    if (!o.hap.vcf.empty() && (!(g_hap_vcf = fopen(o.hap.vcf.c_str(), "w")) || !(g_hap_vcf_lines = tmpfile()))) { fprintf(stderr, "pbdagcon: cannot write %s\n", o.hap.vcf.c_str()); return 1; }
    if (!o.hap_contigs.empty() && !(g_hap_contigs = fopen(o.hap_contigs.c_str(), "w"))) { fprintf(stderr, "pbdagcon: cannot write %s\n", o.hap_contigs.c_str()); return 1; }
    if (!o.hap_windows.empty() && !(g_hap_windows = fopen(o.hap_windows.c_str(), "w"))) { fprintf(stderr, "pbdagcon: cannot write %s\n", o.hap_windows.c_str()); return 1; }
    if (!o.al.alleles.empty() && !(g_site_alleles = fopen(o.al.alleles.c_str(), "w"))) { fprintf(stderr, "pbdagcon: cannot write %s\n", o.al.alleles.c_str()); return 1; }
    if (!o.al.vcf.empty() && (!(g_site_vcf = fopen(o.al.vcf.c_str(), "w")) || !(g_site_vcf_lines = tmpfile()))) { fprintf(stderr, "pbdagcon: cannot write %s\n", o.al.vcf.c_str()); return 1; }
    if (!o.jn.alleles.empty() && !(g_joined_alleles = fopen(o.jn.alleles.c_str(), "w"))) { fprintf(stderr, "pbdagcon: cannot write %s\n", o.jn.alleles.c_str()); return 1; }
    if (!o.jn.vcf.empty() && (!(g_joined_vcf = fopen(o.jn.vcf.c_str(), "w")) || !(g_joined_vcf_lines = tmpfile()))) { fprintf(stderr, "pbdagcon: cannot write %s\n", o.jn.vcf.c_str()); return 1; }
    auto close_pile = [&](int status) {
        // the header of a VCF, now that every target is known, then the records that waited
        auto finish_vcf = [&](FILE *to, FILE *&lines, const std::string &head) {
            bool wrote = fwrite(head.data(), 1, head.size(), to) == head.size();
            rewind(lines);
            char buf[65536];
            for (size_t k; wrote && (k = fread(buf, 1, sizeof buf, lines)) > 0;) wrote = fwrite(buf, 1, k, to) == k;
            if (!wrote || ferror(lines)) g_pile_bad = true;
            fclose(lines); lines = nullptr;
        };
        if (g_site_vcf) {
            std::string head;
            dg_site_vcf_header(head, g_site_vcf_contigs, o.want_phase());
            finish_vcf(g_site_vcf, g_site_vcf_lines, head);
        }
        if (g_joined_vcf) {
            std::string head;
            dg_joined_vcf_header(head, g_joined_vcf_contigs, o.want_phase());
            finish_vcf(g_joined_vcf, g_joined_vcf_lines, head);
        }
        if (g_hap_vcf) {
            std::string head;
            dg_hap_vcf_header(head, g_hap_vcf_contigs);
            finish_vcf(g_hap_vcf, g_hap_vcf_lines, head);
        }
        const std::pair<FILE **, const std::string *> files[] = {{&g_pileup, &o.pile.pileup}, {&g_sites, &o.pile.sites}, {&g_site_reads, &o.sr.site_reads}, {&g_haplotag, &o.sr.haplotag},
                                                                 {&g_site_alleles, &o.al.alleles}, {&g_site_vcf, &o.al.vcf}, {&g_joined_alleles, &o.jn.alleles}, {&g_joined_vcf, &o.jn.vcf},
                                                                 {&g_hap_out, &o.hap.consensus}, {&g_hap_sites, &o.hap.sites}, {&g_hap_vcf, &o.hap.vcf}, {&g_linked_sites, &o.link.linked},
                                                                 {&g_hap_contigs, &o.hap_contigs}, {&g_hap_windows, &o.hap_windows}};
        for (const auto &f : files) {
            if (!*f.first) continue;
            const bool bad = fclose(*f.first) != 0 || g_pile_bad;
            if (bad) { fprintf(stderr, "pbdagcon: error writing %s\n", f.second->c_str()); status = 1; }
            *f.first = nullptr;
        }
        return status;
    };

    // ---- --window: the window driver takes the records from here (windows.h) ----
    if (o.window && !o.dump) {
        DgWinOpts wo{o.min_cov, o.min_len, o.trim, o.window, o.overlap, o.batch_targets, o.fastq, o.verbose, o.devices[0], o.pick, o.edits.empty() ? nullptr : o.edits.c_str(),
                     g_pileup, g_sites, o.pile.min_count, o.pile.min_frac_ppm, g_site_reads, g_haplotag, o.wp};
        wo.link = o.link.on ? &o.link.o : nullptr; wo.linked_sites = g_linked_sites;
        wo.hap_contigs = g_hap_contigs; wo.hap_windows = g_hap_windows; wo.hap_min_sites = o.hap.min_sites; wo.hap_min_reads = o.hap.min_reads;
        if (o.kind == DG_REC_PACKED) { DgBamSource src(bam, ref); return close_pile(dg_run_windows(wo, src, ref)); }
        if (o.kind == DG_REC_PACKED_MD) { DgBamMdSource src(bam, ref); return close_pile(dg_run_windows(wo, src, ref)); }
        if (o.kind == DG_REC_PLAIN_MD) { DgSamMdSource src(in.data, in.size, ref); return close_pile(dg_run_windows(wo, src, ref)); }
        if (o.kind == DG_REC_CS) { DgPafCsSource src(paf); return close_pile(dg_run_windows(wo, src, ref)); }
        if (o.kind == DG_REC_STRANDED) { DgPafSource src(paf); return close_pile(dg_run_windows(wo, src, ref)); }
        DgSamSource src(in.data, in.size, ref);
        return close_pile(dg_run_windows(wo, src, ref));
    }

    // ---- whole targets: the workers start (context creation hides behind the parsing of the first batch), the input
    // is parsed into batches slab by slab, the workers drain ----
    if (!o.edits.empty() && !o.dump && !(g_edits = fopen(o.edits.c_str(), "w"))) { fprintf(stderr, "pbdagcon: cannot write %s\n", o.edits.c_str()); return 1; }
    if (!o.vcf.empty() && !o.dump && (!(g_vcf = fopen(o.vcf.c_str(), "w")) || !(g_vcf_lines = tmpfile()))) { fprintf(stderr, "pbdagcon: cannot write %s\n", o.vcf.c_str()); return 1; }
    Workers wk(o, in.size);
    if (!o.dump) wk.start();
    RecordIndexer rix(in, o, ref, bam, paf);
    TextIndexer tix(in, o);
    int status = o.mode == MODE_RECORDS ? parse_input(rix, first, o, wk) : parse_input(tix, first, o, wk);
    const double t_index = rix.t_index + tix.t_index, t_fill = rix.t_fill + tix.t_fill;
    const double t_parse_end = wall();
    bool fast_exit = false;
    if (!o.dump) {
        const int ws = wk.drain();
        if (ws && !status) status = ws;
        // Every record is printed and the GPU is released: what is left is host-side tidying -- page-locked blobs, the
        // mapping of the input, the HIP runtime's own exit handlers (0.1 - 0.3 s at 1,000 targets) -- which the kernel
        // does for a process that ends, at once.  PBDAGCON_TEARDOWN=1 keeps the orderly way.
        fast_exit = !getenv("PBDAGCON_TEARDOWN") && !status;
    }
    const double t_joined = wall();
    if (!o.dump) dg_report_pick(o.pick, g_over_error, g_over_depth);
    if (g_edits) {
        if (fclose(g_edits) != 0) { fprintf(stderr, "pbdagcon: error writing %s\n", o.edits.c_str()); status = 1; fast_exit = false; }
        if (o.verbose) fprintf(stderr, "pbdagcon: %llu edits written to %s\n", g_n_edits, o.edits.c_str());
    }
    if (g_pileup || g_sites || g_site_reads || g_haplotag || g_linked_sites || g_hap_out || g_hap_sites || g_hap_vcf || g_site_alleles || g_site_vcf || g_joined_alleles || g_joined_vcf) {
        const int ps = close_pile(0);
        if (ps) { status = ps; fast_exit = false; }
    }
    if (g_vcf) {
        std::string head;
        dg_vcf_header(head); head += g_vcf_contigs; dg_vcf_columns(head);
        bool wrote = !g_vcf_bad && fwrite(head.data(), 1, head.size(), g_vcf) == head.size();
        rewind(g_vcf_lines);
        char buf[65536];
        for (size_t k; wrote && (k = fread(buf, 1, sizeof buf, g_vcf_lines)) > 0;) wrote = fwrite(buf, 1, k, g_vcf) == k;
        wrote = wrote && !ferror(g_vcf_lines);
        fclose(g_vcf_lines);
        if (fclose(g_vcf) != 0 || !wrote) { fprintf(stderr, "pbdagcon: error writing %s\n", o.vcf.c_str()); status = 1; fast_exit = false; }
    }
    if (!fast_exit) {
        for (auto &x : wk.bufs) { x.q.release(); x.t.release(); }
        if (in.map) munmap(in.map, in.size);
    }
    fflush(stdout);
    if (g_timing) {
        char teardown[64] = ", no host teardown";
        if (!fast_exit) snprintf(teardown, sizeof teardown, " + teardown %.3f", wall() - t_joined);
        fprintf(stderr, "pbdagcon timing: total %.3f = parse loop %.3f (index %.3f  fill %.3f  wait-for-buffer %.3f) + drain %.3f%s | "
                "worker 0: create %.3f; all workers: flush %.3f (upload %.3f  run %.3f  fetch %.3f)  print %.3f\n",
                wall() - t_main, t_parse_end - t_main, t_index, t_fill, wk.t_wait, t_joined - t_parse_end, teardown, wk.t_create, wk.t_flush,
                g_t_upload, g_t_run, g_t_fetch, wk.t_print);
    }
    if (fast_exit) { fflush(stderr); _exit(0); }
    return status;
}
