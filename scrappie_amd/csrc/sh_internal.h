/* sh_internal.h -- symbols shared between the host C (sh_host.c) and the HIP
 * translation unit (scrappie_hip.hip); not part of the public ABI. */
#ifndef SH_INTERNAL_H
#define SH_INTERNAL_H
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif
float sh_medianf(const float *x, size_t n, float *scratch);
float sh_madf(const float *x, size_t n, const float *med, float *scratch);
int sh_kmerlength(int nstate);
/* homopolymer correction from the 5-row side buffer [nblock][5] = {A,C,G,T homopolymer k-mer, stay} */
int sh_homopolymer_side(const float *side, int *path, int nblock, int nstate);
/* sh_inflate.c: what zlib's uncompress() does (zlib stream -> dst[0 .. cap), *outlen bytes; 0 on success), built for streams of literals */
int sh_zlib_inflate(unsigned char *dst, size_t cap, size_t *outlen, const unsigned char *src, size_t srclen);
unsigned long sh_h5mini_zlib_fallbacks(void);      /* chunks the built-in inflater refused and zlib decoded (expected: 0) */
/* block-based mapping (sh_host.c): are_bounds_sane with its warnings on or off (1 / 0: sane / not) */
int sh_bounds_sane(const size_t *low, const size_t *high, size_t nblock, size_t seqlen, int verbose);
/* packs of candidates (sh_host.c; k_map_pack, sh_map_pack.h): the dynamic LDS a pack of ncell cells and ncand candidates takes -- two
 * rows and a word per cell, ncand + 1 first cells -- under the limit sh_map.h sets for the mapping kernels (the same tokens there) */
#define SH_MAP_LDS 65536
size_t sh_map_pack_lds_bytes(size_t ncell, size_t ncand);
/* windows of the sequence-local CRF mapping (sh_host.c; k_map_crf_local, sh_map_crf_local.h): the dynamic LDS a window of ncell cells takes */
size_t sh_map_crf_local_lds_bytes(size_t ncell);
#define SH_MAP_CRF_LOCAL_CELLS 2034      /* cells of a window at the default stride: 40 952 bytes of LDS, four workgroups per compute unit (160 KB), eight chunks of 256 threads; the fastest measured (profiles/map_crf_local_rate.txt) */
/* windows of the sequence-local transducer mapping (sh_host.c; k_map_local, sh_map_local.h): the dynamic LDS a window of ncell cells of a posterior of
 * nr states takes in the LDS home (head, two columns, three rows and the codes), and in the scratch home (head and columns) */
size_t sh_map_local_lds_bytes(size_t ncell, size_t nr);
size_t sh_map_local_scr_lds_bytes(size_t nr);
#define SH_MAP_LOCAL_CELLS 2798      /* cells of a window at the default stride: with 1025 states 53 152 bytes of LDS, three workgroups per compute unit (160 KB); the fastest measured (profiles/map_local_rate.txt) */
#define SH_MAP_LOCAL_STRIDE 1200     /* the entry positions such a window owned where it was measured (800 blocks): a longer read, which would leave it fewer, takes the largest LDS-resident window */
/* packs of motifs searched inside a flip-flop read (sh_host.c; k_crf_find, sh_crf_find.h): the dynamic LDS a pack of ncell cells takes, with or without positions */
size_t sh_crf_find_lds_bytes(size_t ncell, int pos);
/* packs of candidates a flip-flop read is mapped to (sh_host.c; k_map_crf_pack, sh_map_crf_pack.h): the dynamic LDS a pack of ncell cells takes */
size_t sh_map_crf_pack_lds_bytes(size_t ncell);
/* squiggle matching (sh_host.c): the tables of decode.c:1055-1099 from the host's libm; tab holds 5 npos + 4 floats */
void sh_squiggle_tables(const float *params, size_t npos, size_t ldp, float rate, float prob_back, float *tab, float pens[2]);
/* packs of candidate squiggles of one read (sh_host.c; k_squig_pack, sh_squig_pack.h).  The limit is sh_squig.h's (the same tokens there).
 * Per cell (a position and its back state) LDS holds 11 words: two rows of (position, back) values, loc / scale / logsc / move / stay, and the two
 * words below; per candidate 12: first cell, npos, first piece, pieces, move and stay of START, stay of END, START's two values, END and its step and
 * skip terms; per END piece 4: (value, origin) in two slots.
 *   word A of a cell: its 0-based position in its candidate | its candidate's index in the pack << 12 | SH_SQP_POS0 (position 0: its left neighbour is
 *     START), SH_SQP_POS1 (position 1: START lies two to the left), SH_SQP_RIGHT (position <= npos - 2: it has a right neighbour, is entered by its
 *     back state's source and is an origin of END); a candidate of 1, 2 or 3 positions is the combinations these give
 *   word B of a cell: the END piece it belongs to (index in the pack) | SH_SQP_HEAD where it is the piece's first cell
 * A piece is a candidate's cells inside one group of 64 consecutive cells (one wave of one chunk of 256). */
#define SH_SQ_LDS 65536
/* windows of the reference-local squiggle mapping (sh_host.c; k_squig_local, sh_squig_local.h): the dynamic LDS a window of ncell cells takes in the
 * LDS home and in the scratch home, and the floats of its five rows in device scratch */
size_t sh_squig_local_lds_bytes(size_t ncell);
size_t sh_squig_local_scr_lds_bytes(void);
size_t sh_squig_local_scr_floats(size_t ncell);
#define SH_SQUIG_LOCAL_SCR_MUL 4     /* entry positions per sample a window in device scratch owns at the default stride: two thirds of its cells; the fastest windowed stride on both measured shapes (profiles/squiggle_local_rate.txt) */
#define SH_SQP_CELL_WORDS 11
#define SH_SQP_CAND_WORDS 12
#define SH_SQP_PIECE_WORDS 4
#define SH_SQP_IN_CELL_WORDS 7       /* of those, what the host uploads per cell: the five table entries and the two words */
#define SH_SQP_IN_CAND_WORDS 7       /* ... and per candidate: first cell, npos, first piece, pieces, move[START], stay[START], stay[END] */
#define SH_SQP_POS_MASK 0xfff
#define SH_SQP_CAND_SHIFT 12
#define SH_SQP_POS0 (1 << 24)
#define SH_SQP_POS1 (1 << 25)
#define SH_SQP_RIGHT (1 << 26)
#define SH_SQP_HEAD (1 << 30)
#define SH_SQP_PIECE_MASK 0xfff
size_t sh_squig_pack_lds_bytes(size_t ncell, size_t ncand, size_t npiece);
/* the cell words and piece table of one pack of ncand candidates of npos[k] positions laid end to end: wa / wb [sum npos], piece0 / npiece [ncand]
 * (any may be NULL); returns the pack's pieces */
size_t sh_squig_pack_layout(const size_t *npos, size_t ncand, int *wa, int *wb, int *piece0, int *npiece);
/* dwell correction (sh_host.c): the scale from pos / state (n ints each, `stride` bytes apart), the prior's numerator of an event table, and
 * the whole step on a read the engine holds as arrays (path of n + ntrail entries, n dwells; pos_out may be NULL): the corrected call, the
 * plain one where there is no correction, NULL without a k-mer */
float sh_dwell_scale(const void *pos, const void *state, size_t stride, const int *dwell, int n, float prior_num, size_t basecall_len);
#ifdef SCRAPPIE_HIP_H      /* (event_t: for the files that include scrappie_hip.h first) */
float sh_dwell_prior_num(const event_t *ev, size_t n);
#endif
char *sh_dwell_stitch(const int *path, const int *dwell, int n, int ntrail, int nstate, float prior_num, int *pos_out);
#ifdef SCRAPPIE_HIP_H
/* batched CRF posterior (sh_host.c): is this a 25-row transition matrix with a block; a launch's matrices trans[order[0 .. n)] end to end into dst
 * (NULL: sizes only) with the words of its npad slots and npad / 16 tiles, returns the floats they take; a 5 x (nblock + 1) matrix from [nblock + 1][5] */
int sh_crf_post_ok(const_scrappie_matrix m);
size_t sh_crf_post_stage(const const_scrappie_matrix *trans, const size_t *order, size_t n, size_t npad, float *dst,
                         long long *foff, int *stride, int *T, int *tile_T);
scrappie_matrix sh_crf_post_take(const float *src, size_t nblock);
#endif
#ifdef __cplusplus
}
#endif
#endif
