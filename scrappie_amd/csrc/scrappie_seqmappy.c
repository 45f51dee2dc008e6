/* scrappie_seqmappy.c -- the `scrappie seqmappy` command line over libscrappie_hip.so (src/scrappie_seqmappy.c).
 *
 * Same options, defaults and output as the reference's subcommand: a read's posterior (rgrgr_r94 by default) mapped by
 * local-global Viterbi to the first sequence of a FASTA file, one `block\tpos` line per block.  Added: --model /
 * --model-file / --device as `scrappie raw` takes them, and more `fasta fast5` pairs after the first -- every pair is
 * mapped in ONE scrappie_hip_map_batch call (network, S1 and the mapping on the GPU; only scores and paths return) and
 * the records are written in argument order.  One pair prints exactly what the reference prints.
 * --model rnnrf_r94 (a flip-flop model; the reference refuses it): the global alignment of k_map_crf, the same header
 * line, one record per entry of the path (nblock + 1).
 * --all-records: every record of a pair's FASTA is a candidate for the pair's read, not just the first -- all pairs in ONE
 * scrappie_hip_map_multi_batch call (the network once per read, the candidates packed into workgroups); per pair a table of the
 * records' scores and then the usual header and path of the best one.  Without the option nothing changes.
 * --each-record (flip-flop models): --all-records through scrappie_hip_map_crf_multi_batch (k_map_crf_pack); the same table, then the best
 * record's header and path as plain seqmappy prints them for such a model (nblock + 1 records).  Without the option nothing changes.
 * --inside (flip-flop models): the read lies somewhere INSIDE the sequence -- an amplicon, a plasmid, a chromosome arm.  All pairs
 * in ONE scrappie_hip_map_local_batch call (k_map_crf_local: one workgroup per window of the sequence); the usual header line with
 * `bases first..last` added -- the read spells the record's bases [first, last) -- and nblock + 1 records whose pos is in the
 * record's coordinates (first - 1 while no base is emitted).  Without the option nothing changes.
 * --within (transducer models): the same question for the default models -- all pairs in ONE scrappie_hip_map_post_local_batch call
 * (k_map_local); the transducer output (nblock records, pos -1 in START / END) with `states first..last` added to the header line:
 * the path visits the record's k-mers first .. last - 1.  Without the option nothing changes.
 * --find (flip-flop models): every record of a pair's FASTA is a motif -- a barcode, an adapter, a primer -- searched INSIDE the
 * pair's read.  All pairs in ONE scrappie_hip_find_batch call (k_crf_find: the motifs packed into workgroups); per pair a header
 * line and a table record / name / score / delta / begin / end.  Without the option nothing changes.
 * --edits (flip-flop models): EVERY single-base edit of the first record of a pair's FASTA scored against the pair's read.  All pairs
 * in ONE scrappie_hip_map_crf_edits_batch call (k_crf_edits_rows, k_crf_edits); per pair a header line and one line per position:
 * the base, then del, subA..T and insA..T as differences to the sequence's own Viterbi score.  Without the option nothing changes.
 * --edits --band N: each read mapped to its record with the path first (scrappie_hip_map_batch), then the same table from ONE
 * scrappie_hip_map_crf_edits_banded_batch call in the bands of half-width N around those paths.  Without --band nothing changes.
 * --kmer-edits (transducer models): the same table from ONE scrappie_hip_map_edits_batch call (k_map_edits_rows, k_map_edits), under
 * --stay, --skip and --localpen.
 * --kmer-edits --band N (N >= 1): each read mapped to the record's k-mer states with the path first (scrappie_hip_map_batch), then the same
 * table from ONE scrappie_hip_map_edits_banded_batch call in the bands of half-width N states around those paths.
 */
#define _GNU_SOURCE
#include <getopt.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "scrappie_cli.h"

static void seqmappy_usage(FILE *fh) {
    fputs("Usage: scrappie seqmappy [OPTION...] fasta fast5 [fasta fast5 ...]\n"
          "Scrappie seqmappy (local-global)\n\n"
          "  -l, --localpen=float       Penalty for local matching\n"
          "  -m, --min_prob=probability Minimum bound on probability of match\n"
          "  -o, --output=filename      Write to file rather than stdout\n"
          "  -p, --prefix=string        Prefix to append to name of read\n"
          "      --segmentation=chunk:percentile\n"
          "                             Chunk size and percentile for variance based segmentation\n"
          "  -s, --skip=penalty         Penalty for skipping a base\n"
          "  -y, --stay=penalty         Penalty for staying\n"
          "  -t, --trim=start:end       Number of samples to trim, as start:end\n"
          "      --temperature1=factor  Temperature for softmax weights\n"
          "      --temperature2=factor  Temperature for softmax bias\n"
          "      --licence, --license   Print licensing information\n"
          "      --model=name           Raw model to use (default rgrgr_r94)\n"
          "      --model-file=path      Weight container (.scrm); default $SCRAPPIE_MODEL_DIR/<model>.scrm\n"
          "      --device=N             GPU to run on (default 0)\n"
          "With a flip-flop (CRF) model (--model=rnnrf_r94) the read is aligned globally to the sequence under the model's own\n"
          "transitions: the sequence is encoded with a state length of 1, the penalties are not used, and one record is\n"
          "written per entry of the path (blocks + 1): pos is the last base emitted so far, -1 while none.\n"
          "Every (fasta, fast5) pair is mapped in one batched engine call; records are written in argument order.\n"
          "      --all-records          Map the read to EVERY record of its fasta, not just the first: per pair a line\n"
          "                             `# fast5 to fasta -- N records`, a table record / name / score / per_block (scores\n"
          "                             negated, as in the header line; raw scores: records of different lengths are compared\n"
          "                             as they are), then the header line and the path of the best record, named fasta:name.\n"
          "                             Transducer models only.\n"
          "      --inside               The read lies somewhere inside the sequence (a reference longer than the read): the\n"
          "                             best local placement of the whole read.  `bases first..last` is added to the header\n"
          "                             line -- the read spells bases [first, last) of the record -- and pos is in the\n"
          "                             record's coordinates, first - 1 while none.  Flip-flop (CRF) models only.\n"
          "      --within               --inside for transducer models (the default rgrgr_r94 and its relatives): the best local\n"
          "                             placement of the read in a reference longer than it, under --stay, --skip and\n"
          "                             --localpen.  `states first..last` is added to the header line -- the path visits the\n"
          "                             record's k-mers first .. last - 1, so the read spells bases [first, last + k - 1) -- and\n"
          "                             one record is written per block: pos in the record's coordinates, -1 before the read\n"
          "                             enters the sequence and after it has left.  Not with a flip-flop (CRF) model, --inside,\n"
          "                             --all-records or --find.\n"
          "      --find                 Search every record of the fasta (a barcode, an adapter, a primer) INSIDE the read:\n"
          "                             per pair a line `# fast5 to fasta -- N records, call score S over B blocks, best K`\n"
          "                             and a table record / name / score / delta / begin / end.  score: the best path of\n"
          "                             the whole read that holds the record between entries begin and end (0 .. B; entry t\n"
          "                             is sample t * stride of the trimmed signal), not negated; delta = score - call\n"
          "                             score <= 0, the log-odds against the read's own call; nan where a record cannot be\n"
          "                             searched.  A record is searched as given (no reverse complement).  Flip-flop (CRF)\n"
          "                             models only; not with --inside or --all-records.\n"
          "      --each-record          --all-records for flip-flop (CRF) models (--model=rnnrf_r94): the read against EVERY record\n"
          "                             of its fasta under the model's own transitions (an allele, a haplotype, a reference, an\n"
          "                             edit of the call).  The same line `# fast5 to fasta -- N records` and table record /\n"
          "                             name / score / per_block, then the header line and the path of the best record as plain\n"
          "                             seqmappy prints them for this model (blocks + 1 records), named fasta:name.  Not with a\n"
          "                             transducer model (--all-records), --all-records, --inside, --find or --within.\n"
          "      --edits                Score EVERY single-base edit of the first record of the fasta against the read (Viterbi):\n"
          "                             a line `# fast5 to fasta -- edits of L bases, score S over B blocks` (S not negated), a\n"
          "                             line of column names, then per position i one line pos / base / del / subA subC subG subT /\n"
          "                             insA insC insG insT: the score of the sequence without base i, with base i replaced, and\n"
          "                             with a base inserted BEFORE base i, each as the difference to S (> 0: the edit maps better\n"
          "                             than the sequence; nan: the edited sequence has more bases than the read has entries).\n"
          "                             A last line `L - - - - - - insA..T`: the insertions behind the last base.  An edit's score\n"
          "                             and S are different sums: differences of a few 1e-5 |S| are rounding; confirm an edit with\n"
          "                             --each-record.  Flip-flop (CRF) models only; not with any of the options above.\n"
          "      --band=N               With --edits: map the read to the record first and score the edits inside the band of N cells\n"
          "                             to either side of that path -- a cell of the sequence keeps its band, the edit's own new base\n"
          "                             is free; S is the score inside the band.  The same table for a fraction of the cells; nan\n"
          "                             also where the band leaves an edit no path (a small N at either end of the sequence).  A read\n"
          "                             that cannot be mapped to the record has no path to band around: reported, not scored.\n"
          "      --kmer-edits           The table of --edits for a transducer model (the default rgrgr_r94 and its relatives), under\n"
          "                             --stay, --skip and --localpen: an edit of one base changes up to k consecutive k-mer states\n"
          "                             (nan: the edited sequence admits no path through the read, or has fewer than k bases).\n"
          "                             Confirm an edit with --all-records.  Transducer models only (a flip-flop model: --edits); not\n"
          "                             with any of the options above.\n"
          "                             --kmer-edits --band=N (N >= 1): as --edits --band, in the band of N k-mer states to either side\n"
          "                             of the read's path through the record's states; S is the score of the masked programme.\n", fh);
}

/* --all-records: pair i's read against every record of its FASTA, all pairs in one scrappie_hip_map_multi_batch call; --each-record (crf):
 * the same for a flip-flop model through scrappie_hip_map_crf_multi_batch, the path of nblock + 1 entries */
static int seqmappy_all_records(scrappie_hip_engine *e, int h, int klen, int crf, const scrappie_hip_params *p, char **fasta, size_t npair, FILE *out,
                                int trim_start, int trim_end, int varseg_chunk, float varseg_thresh) {
    raw_table *rts = calloc(npair, sizeof *rts);
    scrappie_hip_map_candidates *cd = calloc(npair, sizeof *cd);
    scrappie_hip_map_multi_result *res = calloc(npair, sizeof *res);
    struct cli_fasta **recs = calloc(npair, sizeof *recs);
    size_t *nrec = calloc(npair, sizeof *nrec);
    int rc = EXIT_SUCCESS;
    for (size_t i = 0; i < npair; i++) {
        const char *fa = fasta[2 * i], *f5 = fasta[2 * i + 1];
        if (cli_read_fasta(fa, &recs[i], &nrec[i], 0) || nrec[i] == 0) { fprintf(stderr, "scrappie: Failed to open \"%s\" for input.\n", fa); rc = EXIT_FAILURE; continue; }
        scrappie_hip_map_target *tg = calloc(nrec[i], sizeof *tg);
        for (size_t k = 0; k < nrec[i]; k++) {           /* a record that cannot be encoded stays an empty candidate: NAN in the table */
            int *codes = recs[i][k].seq ? encode_bases_to_integers(recs[i][k].seq, recs[i][k].n, (size_t)klen) : NULL;
            if (!codes) { fprintf(stderr, "scrappie: cannot encode record %zu of \"%s\": %s\n", k, fa, scrappie_hip_last_error()); continue; }
            tg[k].seq = codes; tg[k].seqlen = recs[i][k].n - (size_t)klen + 1;
        }
        cd[i].cand = tg; cd[i].ncand = nrec[i];
        rts[i] = cli_load_read(f5, trim_start, trim_end, varseg_chunk, varseg_thresh, 1);
        if (!rts[i].raw) { fprintf(stderr, "scrappie: Failed to open \"%s\" for input and trim signal.\n", f5); rc = EXIT_FAILURE; cd[i].ncand = 0; }
    }
    if ((crf ? scrappie_hip_map_crf_multi_batch : scrappie_hip_map_multi_batch)(e, h, rts, cd, npair, p, 1, 1, res) != 0) {
        fprintf(stderr, "scrappie: %s\n", scrappie_hip_last_error());
        rc = EXIT_FAILURE;
    } else {
        for (size_t i = 0; i < npair; i++) {
            if (!rts[i].raw || !cd[i].cand) continue;
            const char *fa = fasta[2 * i], *f5 = fasta[2 * i + 1];
            if (res[i].best < 0 || !res[i].path) { fprintf(stderr, "scrappie: Failed to map \"%s\" to \"%s\"\n", f5, fa); rc = EXIT_FAILURE; continue; }
            const size_t nblock = res[i].nblock;
            fprintf(out, "# %s to %s -- %zu records\n", f5, fa, nrec[i]);
            fprintf(out, "record\tname\tscore\tper_block\n");
            for (size_t k = 0; k < nrec[i]; k++) {
                const float sc = res[i].score[k];
                if (isnan(sc)) fprintf(out, "%zu\t%s\tnan\tnan\n", k, recs[i][k].name ? recs[i][k].name : "");
                else fprintf(out, "%zu\t%s\t%f\t%f\n", k, recs[i][k].name ? recs[i][k].name : "", -sc, -sc / nblock);
            }
            const size_t b = (size_t)res[i].best;
            const float score = res[i].score[b];
            fprintf(out, "# %s to %s:%s -- score %f over %zu blocks (%f per block)\n", f5, fa, recs[i][b].name ? recs[i][b].name : "", -score, nblock, -score / nblock);
            fprintf(out, "block\tpos\n");
            for (size_t t = 0; t < nblock + (crf ? 1 : 0); t++) fprintf(out, "%zu\t%d\n", t, res[i].path[t]);
        }
    }
    scrappie_hip_free_map_multi_results(res, npair);
    for (size_t i = 0; i < npair; i++) {
        if (cd[i].cand) { for (size_t k = 0; k < nrec[i]; k++) free((void *)cd[i].cand[k].seq); free((void *)cd[i].cand); }
        cli_free_fasta(recs[i], nrec[i]);
        free(rts[i].raw); free(rts[i].uuid);
    }
    free(nrec); free(recs); free(res); free(cd); free(rts);
    return rc;
}

/* --find: every record of pair i's FASTA searched inside pair i's read, all pairs in one scrappie_hip_find_batch call */
static int seqmappy_find(scrappie_hip_engine *e, int h, const scrappie_hip_params *p, char **fasta, size_t npair, FILE *out,
                         int trim_start, int trim_end, int varseg_chunk, float varseg_thresh) {
    raw_table *rts = calloc(npair, sizeof *rts);
    scrappie_hip_map_candidates *cd = calloc(npair, sizeof *cd);
    scrappie_hip_find_result *res = calloc(npair, sizeof *res);
    struct cli_fasta **recs = calloc(npair, sizeof *recs);
    size_t *nrec = calloc(npair, sizeof *nrec);
    int rc = EXIT_SUCCESS;
    for (size_t i = 0; i < npair; i++) {
        const char *fa = fasta[2 * i], *f5 = fasta[2 * i + 1];
        if (cli_read_fasta(fa, &recs[i], &nrec[i], 0) || nrec[i] == 0) { fprintf(stderr, "scrappie: Failed to open \"%s\" for input.\n", fa); rc = EXIT_FAILURE; continue; }
        scrappie_hip_map_target *tg = calloc(nrec[i], sizeof *tg);
        for (size_t k = 0; k < nrec[i]; k++) {           /* a record that cannot be encoded stays an empty motif: nan in the table */
            int *codes = recs[i][k].seq && recs[i][k].n ? encode_bases_to_integers(recs[i][k].seq, recs[i][k].n, 1) : NULL;
            if (!codes) { fprintf(stderr, "scrappie: cannot encode record %zu of \"%s\": %s\n", k, fa, scrappie_hip_last_error()); continue; }
            tg[k].seq = codes; tg[k].seqlen = recs[i][k].n;
        }
        cd[i].cand = tg; cd[i].ncand = nrec[i];
        rts[i] = cli_load_read(f5, trim_start, trim_end, varseg_chunk, varseg_thresh, 1);
        if (!rts[i].raw) { fprintf(stderr, "scrappie: Failed to open \"%s\" for input and trim signal.\n", f5); rc = EXIT_FAILURE; cd[i].ncand = 0; }
    }
    if (scrappie_hip_find_batch(e, h, rts, cd, npair, p, 1, res) != 0) {
        fprintf(stderr, "scrappie: %s\n", scrappie_hip_last_error());
        rc = EXIT_FAILURE;
    } else {
        for (size_t i = 0; i < npair; i++) {
            if (!rts[i].raw || !cd[i].cand) continue;
            const char *fa = fasta[2 * i], *f5 = fasta[2 * i + 1];
            if (res[i].nblock == 0 || isnan(res[i].call_score)) { fprintf(stderr, "scrappie: Failed to search \"%s\" for \"%s\"\n", f5, fa); rc = EXIT_FAILURE; continue; }
            fprintf(out, "# %s to %s -- %zu records, call score %f over %zu blocks, best %d\n", f5, fa, nrec[i], res[i].call_score, res[i].nblock, res[i].best);
            fprintf(out, "record\tname\tscore\tdelta\tbegin\tend\n");
            for (size_t k = 0; k < nrec[i]; k++) {
                const float sc = res[i].score[k];
                if (isnan(sc)) fprintf(out, "%zu\t%s\tnan\tnan\t-1\t-1\n", k, recs[i][k].name ? recs[i][k].name : "");
                else fprintf(out, "%zu\t%s\t%f\t%f\t%d\t%d\n", k, recs[i][k].name ? recs[i][k].name : "", sc, sc - res[i].call_score, (int)res[i].begin[k], (int)res[i].end[k]);
            }
        }
    }
    scrappie_hip_free_find_results(res, npair);
    for (size_t i = 0; i < npair; i++) {
        if (cd[i].cand) { for (size_t k = 0; k < nrec[i]; k++) free((void *)cd[i].cand[k].seq); free((void *)cd[i].cand); }
        cli_free_fasta(recs[i], nrec[i]);
        free(rts[i].raw); free(rts[i].uuid);
    }
    free(nrec); free(recs); free(res); free(cd); free(rts);
    return rc;
}

/* an edit's score as its difference to the sequence's own, "nan" where the edit has no admissible path */
static void print_delta(FILE *out, float score, float base) {
    if (isnan(score)) fputs("\tnan", out);
    else fprintf(out, "\t%f", score - base);
}

/* --edits --band: the nb reads mapped to their sequences with the path in one scrappie_hip_map_batch call (k_map_crf), and around each path the band
 * of that half-width (scrappie_hip_map_crf_path_band) as the target's poslow / poshigh.  Returns the 2 nb arrays to free -- low and high of entry m at
 * [2 m], [2 m + 1]; a pair that cannot be mapped keeps no band (poslow stays NULL), and the caller reports it as not scored --, NULL where the call failed
 * (scrappie_hip_last_error() says why). */
static size_t **seqmappy_path_bands(scrappie_hip_engine *e, int h, const scrappie_hip_params *p, const raw_table *rts, scrappie_hip_map_target *tg,
                                    size_t nb, size_t halfwidth) {
    scrappie_hip_map_result *mp = calloc(nb, sizeof *mp);
    size_t **bands = calloc(2 * nb, sizeof *bands);
    if (!mp || !bands || scrappie_hip_map_batch(e, h, rts, tg, nb, p, 1, 1, mp) != 0) {
        free(mp); free(bands);              /* (a failed call has released its results) */
        return NULL;
    }
    for (size_t i = 0; i < nb; i++) {
        if (!mp[i].path) continue;
        size_t *lo = malloc((mp[i].nblock + 1) * sizeof *lo), *hi = malloc((mp[i].nblock + 1) * sizeof *hi);
        if (lo && hi && scrappie_hip_map_crf_path_band(mp[i].path, mp[i].nblock, tg[i].seqlen, halfwidth, lo, hi) == 0) {
            bands[2 * i] = lo; bands[2 * i + 1] = hi;
            tg[i].poslow = lo; tg[i].poshigh = hi;
        } else { free(lo); free(hi); }
    }
    scrappie_hip_free_map_results(mp, nb);
    free(mp);
    return bands;
}

/* --kmer-edits --band: the same for a transducer model of k-mers of klen bases.  The reads are mapped to the k-mer states of their sequences
 * (scrappie_hip_map_batch, k_map: a path of nblock entries), the band of that half-width in states goes around each path
 * (scrappie_hip_map_path_band) and becomes poslow / poshigh of the target tg[i], whose sequence stays the BASES.  A sequence shorter than a k-mer is
 * mapped as an empty one: it gets no band and the edits call refuses it by its own rule. */
static size_t **seqmappy_kmer_path_bands(scrappie_hip_engine *e, int h, const scrappie_hip_params *p, const raw_table *rts, scrappie_hip_map_target *tg,
                                         size_t nb, size_t halfwidth, int klen) {
    scrappie_hip_map_result *mp = calloc(nb, sizeof *mp);
    scrappie_hip_map_target *st = calloc(nb, sizeof *st);
    int **states = calloc(nb, sizeof *states);
    size_t **bands = calloc(2 * nb, sizeof *bands);
    int ok = mp && st && states && bands;
    for (size_t i = 0; ok && i < nb; i++) {
        if (tg[i].seqlen < (size_t)klen) continue;
        const size_t ns = tg[i].seqlen - (size_t)klen + 1;
        if (!(states[i] = malloc(ns * sizeof **states))) { ok = 0; break; }
        for (size_t q = 0; q < ns; q++) {                    /* the first base the most significant (encode_bases_to_integers) */
            int code = 0;
            for (int j = 0; j < klen; j++) code = code * 4 + tg[i].seq[q + (size_t)j];
            states[i][q] = code;
        }
        st[i].seq = states[i]; st[i].seqlen = ns;
    }
    if (ok && scrappie_hip_map_batch(e, h, rts, st, nb, p, 1, 1, mp) != 0) ok = 0;      /* (a failed call has released its results) */
    for (size_t i = 0; ok && i < nb; i++) {
        if (!mp[i].path || !st[i].seqlen) continue;
        size_t *lo = malloc(mp[i].nblock * sizeof *lo), *hi = malloc(mp[i].nblock * sizeof *hi);
        if (lo && hi && scrappie_hip_map_path_band(mp[i].path, mp[i].nblock, st[i].seqlen, halfwidth, lo, hi) == 0) {
            bands[2 * i] = lo; bands[2 * i + 1] = hi;
            tg[i].poslow = lo; tg[i].poshigh = hi;
        } else { free(lo); free(hi); }
    }
    if (ok) scrappie_hip_free_map_results(mp, nb);
    for (size_t i = 0; states && i < nb; i++) free(states[i]);
    free(states); free(st); free(mp);
    if (!ok) { free(bands); return NULL; }
    return bands;
}

/* --edits (klen 0) and --kmer-edits (klen: the bases of the transducer model's k-mer): every single-base edit of the first record of pair i's FASTA
 * against pair i's read, all pairs in one scrappie_hip_map_crf_edits_batch or scrappie_hip_map_edits_batch call; band >= 0 (--band): the flip-flop
 * table from scrappie_hip_map_crf_edits_banded_batch, the transducer one from scrappie_hip_map_edits_banded_batch, in the bands of that half-width
 * around the reads' Viterbi paths */
static int seqmappy_edits(scrappie_hip_engine *e, int h, const scrappie_hip_params *p, char **fasta, size_t npair, FILE *out,
                          int trim_start, int trim_end, int varseg_chunk, float varseg_thresh, int klen, long band) {
    const char *const opt = klen ? "--kmer-edits" : "--edits";
    size_t **bands = NULL;                  /* --band (band >= 0): low and high of entry m at bands[2 m], bands[2 m + 1] */
    /* entry m of the batch is pair who[m]: a pair whose fasta or fast5 did not load is reported here and never reaches the engine */
    raw_table *rts = calloc(npair, sizeof *rts);
    scrappie_hip_map_target *tg = calloc(npair, sizeof *tg);
    scrappie_hip_edits_result *res = calloc(npair, sizeof *res);
    int **codes = calloc(npair, sizeof *codes);
    size_t *who = calloc(npair, sizeof *who), nb = 0;
    int rc = EXIT_SUCCESS;
    for (size_t j = 0; j < npair; j++) {
        const char *fa = fasta[2 * j], *f5 = fasta[2 * j + 1];
        struct cli_fasta *rec = NULL;       /* the first record of the file */
        size_t nrec = 0;
        if (cli_read_fasta(fa, &rec, &nrec, 1) || nrec == 0 || !rec[0].seq || rec[0].n == 0) { fprintf(stderr, "scrappie: Failed to open \"%s\" for input.\n", fa); cli_free_fasta(rec, nrec); rc = EXIT_FAILURE; continue; }
        const size_t n = rec[0].n;
        int *cd = encode_bases_to_integers(rec[0].seq, n, 1);
        cli_free_fasta(rec, nrec);
        if (!cd) { fprintf(stderr, "scrappie: cannot encode the sequence of \"%s\": %s\n", fa, scrappie_hip_last_error()); rc = EXIT_FAILURE; continue; }
        const raw_table rt = cli_load_read(f5, trim_start, trim_end, varseg_chunk, varseg_thresh, 1);
        if (!rt.raw) { fprintf(stderr, "scrappie: Failed to open \"%s\" for input and trim signal.\n", f5); free(cd); rc = EXIT_FAILURE; continue; }
        codes[nb] = cd; tg[nb].seq = cd; tg[nb].seqlen = n; rts[nb] = rt; who[nb] = j;
        nb++;
    }
    int failed = 0;                         /* a batch call failed as a whole: its text is the engine's */
    if (nb && band >= 0 && !(bands = klen ? seqmappy_kmer_path_bands(e, h, p, rts, tg, nb, (size_t)band, klen) : seqmappy_path_bands(e, h, p, rts, tg, nb, (size_t)band))) failed = 1;
    if (nb && !failed)
        failed = (klen ? (band >= 0 ? scrappie_hip_map_edits_banded_batch(e, h, rts, tg, nb, p, 1, res) : scrappie_hip_map_edits_batch(e, h, rts, tg, nb, p, 1, res)) :
                  band >= 0 ? scrappie_hip_map_crf_edits_banded_batch(e, h, rts, tg, nb, p, 1, res) : scrappie_hip_map_crf_edits_batch(e, h, rts, tg, nb, p, 1, res)) != 0;
    if (failed) {
        fprintf(stderr, "scrappie: %s\n", scrappie_hip_last_error());
        rc = EXIT_FAILURE;
    } else {
        const size_t maxL = klen ? scrappie_hip_map_edits_max_bases((size_t)klen) : scrappie_hip_map_crf_lds_max_seq();
        for (size_t i = 0; i < nb; i++) {
            const char *fa = fasta[2 * who[i]], *f5 = fasta[2 * who[i] + 1];
            if (isnan(res[i].base)) {        /* the engine's error text names the call's FIRST refusal only: this pair's own reason is worked out here */
                if (tg[i].seqlen > maxL) fprintf(stderr, "scrappie: Failed to score the edits of \"%s\" for \"%s\": %zu bases are too long for %s (at most %zu: pass a window of the sequence)\n", fa, f5, tg[i].seqlen, opt, maxL);
                else if (tg[i].seqlen < (size_t)klen) fprintf(stderr, "scrappie: Failed to score the edits of \"%s\" for \"%s\": %zu bases are shorter than the model's k-mer (%d)\n", fa, f5, tg[i].seqlen, klen);
                else fprintf(stderr, "scrappie: Failed to score the edits of \"%s\" for \"%s\": the read cannot be run (too short for the model, or its signal is out of range)\n", fa, f5);
                rc = EXIT_FAILURE;
                continue;
            }
            if (band >= 0 && !tg[i].poslow) {   /* no path to build the band around: what the call scored for it is unbanded, and is not printed as --band's */
                fprintf(stderr, "scrappie: Failed to score the edits of \"%s\" for \"%s\" in a band: the read cannot be mapped to the sequence (no admissible path), so there is no path for --band; not scored\n", fa, f5);
                rc = EXIT_FAILURE;
                continue;
            }
            const size_t L = res[i].seqlen;
            const float base = res[i].base;
            fprintf(out, "# %s to %s -- edits of %zu bases, score %f over %zu blocks\n", f5, fa, L, base, res[i].nblock);
            fprintf(out, "pos\tbase\tdel\tsubA\tsubC\tsubG\tsubT\tinsA\tinsC\tinsG\tinsT\n");
            for (size_t k = 0; k <= L; k++) {
                if (k < L) {
                    fprintf(out, "%zu\t%c", k, "ACGT"[codes[i][k]]);
                    print_delta(out, res[i].del[k], base);
                    for (int c = 0; c < 4; c++) print_delta(out, res[i].sub[4 * k + c], base);
                } else fprintf(out, "%zu\t-\t-\t-\t-\t-\t-", k);
                for (int c = 0; c < 4; c++) print_delta(out, res[i].ins[4 * k + c], base);
                fputc('\n', out);
            }
        }
    }
    scrappie_hip_free_edits_results(res, nb);
    for (size_t i = 0; i < nb; i++) { free(codes[i]); free(rts[i].raw); free(rts[i].uuid); }
    for (size_t i = 0; bands && i < 2 * nb; i++) free(bands[i]);
    free(bands); free(who); free(codes); free(res); free(tg); free(rts);
    return rc;
}

/* --inside: pair i's read into the first record of its FASTA, all pairs in one scrappie_hip_map_local_batch call; --within (klen: the
 * transducer model's k-mer length, 0 for --inside): the same through scrappie_hip_map_post_local_batch */
static int seqmappy_inside(scrappie_hip_engine *e, int h, int klen, const scrappie_hip_params *p, char **fasta, size_t npair, FILE *out,
                           int trim_start, int trim_end, int varseg_chunk, float varseg_thresh) {
    raw_table *rts = calloc(npair, sizeof *rts);
    scrappie_hip_map_local_target *tg = calloc(npair, sizeof *tg);
    scrappie_hip_map_local_result *res = calloc(npair, sizeof *res);
    int **codes = calloc(npair, sizeof *codes);
    int rc = EXIT_SUCCESS;
    for (size_t i = 0; i < npair; i++) {
        const char *fa = fasta[2 * i], *f5 = fasta[2 * i + 1];
        struct cli_fasta *rec = NULL;       /* the first record of the file */
        size_t nrec = 0;
        if (cli_read_fasta(fa, &rec, &nrec, 1) || nrec == 0 || !rec[0].seq || rec[0].n == 0) { fprintf(stderr, "scrappie: Failed to open \"%s\" for input.\n", fa); cli_free_fasta(rec, nrec); rc = EXIT_FAILURE; continue; }
        const size_t n = rec[0].n, k = klen ? (size_t)klen : 1;
        codes[i] = encode_bases_to_integers(rec[0].seq, n, k);
        cli_free_fasta(rec, nrec);
        if (!codes[i]) { fprintf(stderr, "scrappie: cannot encode the sequence of \"%s\": %s\n", fa, scrappie_hip_last_error()); rc = EXIT_FAILURE; continue; }
        tg[i].seq = codes[i]; tg[i].seqlen = n - k + 1;
        rts[i] = cli_load_read(f5, trim_start, trim_end, varseg_chunk, varseg_thresh, 1);
        if (!rts[i].raw) { fprintf(stderr, "scrappie: Failed to open \"%s\" for input and trim signal.\n", f5); rc = EXIT_FAILURE; continue; }
    }
    if ((klen ? scrappie_hip_map_post_local_batch : scrappie_hip_map_local_batch)(e, h, rts, tg, npair, p, 1, 1, res) != 0) {
        fprintf(stderr, "scrappie: %s\n", scrappie_hip_last_error());
        rc = EXIT_FAILURE;
    } else {
        for (size_t i = 0; i < npair; i++) {
            if (!rts[i].raw || !codes[i]) continue;
            if (!res[i].path) { fprintf(stderr, "scrappie: Failed to map \"%s\" to \"%s\"\n", fasta[2 * i + 1], fasta[2 * i]); rc = EXIT_FAILURE; continue; }
            const float score = res[i].score;
            const size_t nblock = res[i].nblock;
            fprintf(out, "# %s to %s -- score %f over %zu blocks (%f per block) %s %zu..%zu\n", fasta[2 * i + 1], fasta[2 * i], -score, nblock, -score / nblock,
                    klen ? "states" : "bases", res[i].first, res[i].last);
            fprintf(out, "block\tpos\n");
            for (size_t b = 0; b < nblock + (klen ? 0 : 1); b++) fprintf(out, "%zu\t%d\n", b, res[i].path[b]);
        }
    }
    scrappie_hip_free_map_local_results(res, npair);
    for (size_t i = 0; i < npair; i++) { free(codes[i]); free(rts[i].raw); free(rts[i].uuid); }
    free(codes); free(res); free(tg); free(rts);
    return rc;
}

int main_seqmappy(int argc, char **argv) {
    enum { O_SEG = 256, O_T1, O_T2, O_LIC, O_MODEL, O_MFILE, O_DEV, O_ALL, O_INSIDE, O_FIND, O_WITHIN, O_EACH, O_EDITS, O_KEDITS, O_BAND };
    static const struct option lo[] = {
        {"localpen", 1, 0, 'l'}, {"min_prob", 1, 0, 'm'}, {"output", 1, 0, 'o'}, {"prefix", 1, 0, 'p'},
        {"segmentation", 1, 0, O_SEG}, {"skip", 1, 0, 's'}, {"stay", 1, 0, 'y'}, {"trim", 1, 0, 't'},
        {"temperature1", 1, 0, O_T1}, {"temperature2", 1, 0, O_T2}, {"licence", 0, 0, O_LIC}, {"license", 0, 0, O_LIC},
        {"model", 1, 0, O_MODEL}, {"model-file", 1, 0, O_MFILE}, {"device", 1, 0, O_DEV}, {"all-records", 0, 0, O_ALL}, {"inside", 0, 0, O_INSIDE}, {"find", 0, 0, O_FIND}, {"within", 0, 0, O_WITHIN}, {"each-record", 0, 0, O_EACH}, {"edits", 0, 0, O_EDITS}, {"kmer-edits", 0, 0, O_KEDITS}, {"band", 1, 0, O_BAND}, {"help", 0, 0, '?'}, {0, 0, 0, 0}};
    int all_records = 0, inside = 0, find = 0, within = 0, each_record = 0, edits = 0, kmer_edits = 0;
    long band = -1;                         /* --band: the half-width in cells; -1: no band */
    /* defaults: scrappie_seqmappy.c:62-78 */
    scrappie_hip_params p = scrappie_hip_default_params();
    p.local_pen = 4.0f; p.min_prob = 1e-5f; p.stay_pen = 0.0f; p.skip_pen = 0.0f; p.tempW = 1.0f; p.tempb = 1.0f;
    FILE *out = stdout;
    int trim_start = 200, trim_end = 10, varseg_chunk = 100, device = 0;
    float varseg_thresh = 0.0f;
    const char *model = "rgrgr_r94", *model_file = NULL;
    double pct;
    int c;
    optind = 1;
    while ((c = getopt_long(argc, argv, "l:m:o:p:s:y:t:", lo, NULL)) != -1) {
        switch (c) {
        case 'l': p.local_pen = (float)atof(optarg); break;
        case 'm': p.min_prob = (float)atof(optarg); break;
        case 'o': if (!(out = cli_open_output(optarg))) return EXIT_FAILURE; break;
        case 'p': break;                 /* accepted; the reference's seqmappy never prints it */
        case 's': p.skip_pen = (float)atof(optarg); break;
        case 'y': p.stay_pen = (float)atof(optarg); break;
        case 't': if (cli_parse_trim(optarg, &trim_start, &trim_end)) { fprintf(stderr, "scrappie: --trim wants start:end\n"); return EXIT_FAILURE; } break;
        case O_SEG:
            if (cli_parse_segmentation(optarg, &varseg_chunk, &pct) || varseg_chunk < 0 || pct <= 0 || pct >= 100) { fprintf(stderr, "scrappie: --segmentation should be of form chunk:percentile\n"); return EXIT_FAILURE; }
            varseg_thresh = (float)(pct / 100.0); break;
        case O_T1: p.tempW = (float)atof(optarg); break;
        case O_T2: p.tempb = (float)atof(optarg); break;
        case O_LIC: cli_licence(); break;
        case O_MODEL:
            if (get_raw_model(optarg) == SCRAPPIE_MODEL_INVALID) { fprintf(stderr, "scrappie: Invalid model name \"%s\"\n", optarg); return EXIT_FAILURE; }
            model = optarg;
            break;
        case O_MFILE: model_file = optarg; break;
        case O_DEV: device = atoi(optarg); break;
        case O_ALL: all_records = 1; break;
        case O_INSIDE: inside = 1; break;
        case O_FIND: find = 1; break;
        case O_WITHIN: within = 1; break;
        case O_EACH: each_record = 1; break;
        case O_EDITS: edits = 1; break;
        case O_KEDITS: kmer_edits = 1; break;
        case O_BAND: {
            char *end = NULL;
            band = strtol(optarg, &end, 10);
            if (end == optarg || *end || band < 0) { fprintf(stderr, "scrappie: --band wants a half-width in cells, 0 or more\n"); return EXIT_FAILURE; }
            break;
        }
        default: seqmappy_usage(stderr); return EXIT_FAILURE;
        }
    }
    const int nargs = argc - optind;
    if (nargs <= 0) { seqmappy_usage(stderr); return EXIT_FAILURE; }
    if (nargs % 2) { fprintf(stderr, "scrappie: fast5 file is a required argument\n"); return EXIT_FAILURE; }    /* scrappie_seqmappy.c:153 */
    const size_t npair = (size_t)nargs / 2;
    if (band >= 0 && !edits && !kmer_edits) { fprintf(stderr, "scrappie: --band is the band of --edits (a transducer model: of --kmer-edits); it needs --edits\n"); return EXIT_FAILURE; }
    if (band == 0 && kmer_edits) {
        fprintf(stderr, "scrappie: --kmer-edits --band wants a half-width of at least 1 state: a skip moves two states, so a half-width of 0 cannot hold a path\n");
        return EXIT_FAILURE;
    }
    if (kmer_edits && (edits || all_records || inside || find || within || each_record)) {
        fprintf(stderr, "scrappie: --kmer-edits scores every single-base edit of the first record of a fasta; it cannot be combined with %s\n",
                edits ? "--edits" : all_records ? "--all-records" : inside ? "--inside" : find ? "--find" : within ? "--within" : "--each-record");
        return EXIT_FAILURE;
    }
    if (kmer_edits && get_raw_model(model) == SCRAPPIE_MODEL_RNNRF_R9_4) {
        fprintf(stderr, "scrappie: --kmer-edits scores reads of transducer models only; \"%s\" is a flip-flop (CRF) model (--edits)\n", model);
        return EXIT_FAILURE;
    }
    if (edits && (all_records || inside || find || within || each_record)) {
        fprintf(stderr, "scrappie: --edits scores every single-base edit of the first record of a fasta; it cannot be combined with %s\n",
                all_records ? "--all-records" : inside ? "--inside" : find ? "--find" : within ? "--within" : "--each-record");
        return EXIT_FAILURE;
    }
    if (edits && get_raw_model(model) != SCRAPPIE_MODEL_RNNRF_R9_4) {
        fprintf(stderr, "scrappie: --edits scores reads of flip-flop (CRF) models only (--model=rnnrf_r94); \"%s\" is a transducer model\n", model);
        return EXIT_FAILURE;
    }
    if (each_record && (all_records || inside || find || within)) {
        fprintf(stderr, "scrappie: --each-record maps a read of a flip-flop (CRF) model to every record of its fasta; it cannot be combined with %s\n",
                all_records ? "--all-records" : inside ? "--inside" : find ? "--find" : "--within");
        return EXIT_FAILURE;
    }
    if (each_record && get_raw_model(model) != SCRAPPIE_MODEL_RNNRF_R9_4) {
        fprintf(stderr, "scrappie: --each-record maps flip-flop (CRF) models only (--model=rnnrf_r94); \"%s\" is a transducer model (--all-records)\n", model);
        return EXIT_FAILURE;
    }
    if (within && (inside || all_records || find)) {
        fprintf(stderr, "scrappie: --within maps a read of a transducer model into the first record of its fasta; it cannot be combined with %s\n",
                inside ? "--inside" : all_records ? "--all-records" : "--find");
        return EXIT_FAILURE;
    }
    if (within && get_raw_model(model) == SCRAPPIE_MODEL_RNNRF_R9_4) {
        fprintf(stderr, "scrappie: --within maps transducer models only; \"%s\" is a flip-flop (CRF) model (--inside)\n", model);
        return EXIT_FAILURE;
    }
    if (find && inside) { fprintf(stderr, "scrappie: --find searches the records of a fasta inside the read; it cannot be combined with --inside\n"); return EXIT_FAILURE; }
    if (find && all_records) { fprintf(stderr, "scrappie: --find searches every record of a fasta already; it cannot be combined with --all-records\n"); return EXIT_FAILURE; }
    if (find && get_raw_model(model) != SCRAPPIE_MODEL_RNNRF_R9_4) {
        fprintf(stderr, "scrappie: --find searches reads of flip-flop (CRF) models only (--model=rnnrf_r94); \"%s\" is a transducer model\n", model);
        return EXIT_FAILURE;
    }
    if (inside && all_records) { fprintf(stderr, "scrappie: --inside maps a read into the first record of its fasta; it cannot be combined with --all-records\n"); return EXIT_FAILURE; }
    if (inside && get_raw_model(model) != SCRAPPIE_MODEL_RNNRF_R9_4) {
        fprintf(stderr, "scrappie: --inside maps flip-flop (CRF) models only (--model=rnnrf_r94); \"%s\" is a transducer model\n", model);
        return EXIT_FAILURE;
    }
    if (all_records && get_raw_model(model) == SCRAPPIE_MODEL_RNNRF_R9_4) {
        fprintf(stderr, "scrappie: --all-records maps transducer models only; \"%s\" is a flip-flop (CRF) model\n", model);
        return EXIT_FAILURE;
    }
    char **fasta = argv + optind;        /* fasta[2 i], fast5 = fasta[2 i + 1] */

    int h;
    scrappie_hip_engine *e = cli_open_model(device, model, model_file, &h);
    if (!e) return EXIT_FAILURE;
    int nstate = scrappie_hip_model_states(e, h), klen = 0;
    const int crf = nstate == 25;        /* a flip-flop model (rnnrf_r94): bases as states of length 1, a path of nblock + 1 entries */
    if (crf) klen = 1;
    else for (int nk = nstate - 1; nk > 1 && nk % 4 == 0; nk /= 4) klen++;
    if (edits) {
        int rc = EXIT_FAILURE;
        if (!crf) fprintf(stderr, "scrappie: --edits scores reads of flip-flop (CRF) models only; \"%s\" is a transducer model\n", model);
        else rc = seqmappy_edits(e, h, &p, fasta, npair, out, trim_start, trim_end, varseg_chunk, varseg_thresh, 0, band);
        if (out != stdout) fclose(out);
        scrappie_hip_engine_destroy(e);
        return rc;
    }
    if (kmer_edits) {
        int rc = EXIT_FAILURE;
        if (crf) fprintf(stderr, "scrappie: --kmer-edits scores reads of transducer models only; \"%s\" is a flip-flop (CRF) model (--edits)\n", model);
        else rc = seqmappy_edits(e, h, &p, fasta, npair, out, trim_start, trim_end, varseg_chunk, varseg_thresh, klen, band);
        if (out != stdout) fclose(out);
        scrappie_hip_engine_destroy(e);
        return rc;
    }
    if (find) {
        int rc = EXIT_FAILURE;
        if (!crf) fprintf(stderr, "scrappie: --find searches reads of flip-flop (CRF) models only; \"%s\" is a transducer model\n", model);
        else rc = seqmappy_find(e, h, &p, fasta, npair, out, trim_start, trim_end, varseg_chunk, varseg_thresh);
        if (out != stdout) fclose(out);
        scrappie_hip_engine_destroy(e);
        return rc;
    }
    if (inside) {
        int rc = EXIT_FAILURE;
        if (!crf) fprintf(stderr, "scrappie: --inside maps flip-flop (CRF) models only; \"%s\" is a transducer model\n", model);
        else rc = seqmappy_inside(e, h, 0, &p, fasta, npair, out, trim_start, trim_end, varseg_chunk, varseg_thresh);
        if (out != stdout) fclose(out);
        scrappie_hip_engine_destroy(e);
        return rc;
    }
    if (within) {
        int rc = EXIT_FAILURE;
        if (crf) fprintf(stderr, "scrappie: --within maps transducer models only; \"%s\" is a flip-flop (CRF) model (--inside)\n", model);
        else rc = seqmappy_inside(e, h, klen, &p, fasta, npair, out, trim_start, trim_end, varseg_chunk, varseg_thresh);
        if (out != stdout) fclose(out);
        scrappie_hip_engine_destroy(e);
        return rc;
    }
    if (all_records) {
        int rc = EXIT_FAILURE;
        if (crf) fprintf(stderr, "scrappie: --all-records maps transducer models only; \"%s\" is a flip-flop (CRF) model\n", model);
        else rc = seqmappy_all_records(e, h, klen, 0, &p, fasta, npair, out, trim_start, trim_end, varseg_chunk, varseg_thresh);
        if (out != stdout) fclose(out);
        scrappie_hip_engine_destroy(e);
        return rc;
    }
    if (each_record) {
        int rc = EXIT_FAILURE;
        if (!crf) fprintf(stderr, "scrappie: --each-record maps flip-flop (CRF) models only; \"%s\" is a transducer model (--all-records)\n", model);
        else rc = seqmappy_all_records(e, h, 1, 1, &p, fasta, npair, out, trim_start, trim_end, varseg_chunk, varseg_thresh);
        if (out != stdout) fclose(out);
        scrappie_hip_engine_destroy(e);
        return rc;
    }

    raw_table *rts = calloc(npair, sizeof *rts);
    scrappie_hip_map_target *tg = calloc(npair, sizeof *tg);
    scrappie_hip_map_result *res = calloc(npair, sizeof *res);
    int **codes = calloc(npair, sizeof *codes);
    int rc = EXIT_SUCCESS;
    for (size_t i = 0; i < npair; i++) {
        const char *fa = fasta[2 * i], *f5 = fasta[2 * i + 1];
        struct cli_fasta *rec = NULL;       /* the first record of the file */
        size_t nrec = 0;
        if (cli_read_fasta(fa, &rec, &nrec, 1) || nrec == 0 || !rec[0].seq || rec[0].n == 0) { fprintf(stderr, "scrappie: Failed to open \"%s\" for input.\n", fa); cli_free_fasta(rec, nrec); rc = EXIT_FAILURE; continue; }
        const size_t n = rec[0].n;
        codes[i] = encode_bases_to_integers(rec[0].seq, n, (size_t)klen);
        cli_free_fasta(rec, nrec);
        if (!codes[i]) { fprintf(stderr, "scrappie: cannot encode the sequence of \"%s\": %s\n", fa, scrappie_hip_last_error()); rc = EXIT_FAILURE; continue; }
        tg[i].seq = codes[i]; tg[i].seqlen = n - (size_t)klen + 1;
        /* scrappie_seqmappy.c:187-194 */
        rts[i] = cli_load_read(f5, trim_start, trim_end, varseg_chunk, varseg_thresh, 1);
        if (!rts[i].raw) { fprintf(stderr, "scrappie: Failed to open \"%s\" for input and trim signal.\n", f5); rc = EXIT_FAILURE; continue; }
    }
    if (scrappie_hip_map_batch(e, h, rts, tg, npair, &p, 1, 1, res) != 0) {
        fprintf(stderr, "scrappie: %s\n", scrappie_hip_last_error());
        rc = EXIT_FAILURE;
    } else {
        for (size_t i = 0; i < npair; i++) {
            if (!rts[i].raw || !codes[i]) continue;
            if (!res[i].path) { fprintf(stderr, "scrappie: Failed to map \"%s\" to \"%s\"\n", fasta[2 * i + 1], fasta[2 * i]); rc = EXIT_FAILURE; continue; }
            const float score = res[i].score;
            const size_t nblock = res[i].nblock;
            fprintf(out, "# %s to %s -- score %f over %zu blocks (%f per block)\n", fasta[2 * i + 1], fasta[2 * i], -score, nblock, -score / nblock);
            fprintf(out, "block\tpos\n");
            for (size_t b = 0; b < nblock + (crf ? 1 : 0); b++) fprintf(out, "%zu\t%d\n", b, res[i].path[b]);
        }
    }
    scrappie_hip_free_map_results(res, npair);
    for (size_t i = 0; i < npair; i++) { free(codes[i]); free(rts[i].raw); free(rts[i].uuid); }
    free(codes); free(res); free(tg); free(rts);
    if (out != stdout) fclose(out);
    scrappie_hip_engine_destroy(e);
    return rc;
}
