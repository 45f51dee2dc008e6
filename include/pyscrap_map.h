/* include/pyscrap_map.h -- the block-based mapping prototypes of the reference's python/pyscrap.h (lines 41-58 and 61),
 * verbatim: appended to the cdef text of include/pyscrap_raw.h they route scrappy.map_post_to_sequence to this library
 * (option A). */

// Block-based mapping
bool are_bounds_sane(size_t const * low, size_t const * high,
                     size_t nblock, size_t seqlen);
float map_to_sequence_forward(const_scrappie_matrix logpost,
                              float stay_pen, float skip_pen, float local_pen,
                              int const *seq, size_t seqlen);
float map_to_sequence_forward_banded(const_scrappie_matrix logpost,
                                     float stay_pen, float skip_pen, float local_pen,
                                     int const *seq, size_t seqlen,
                                     size_t const * poslow, size_t const * poshigh);

float map_to_sequence_viterbi(const_scrappie_matrix logpost,
                              float stay_pen, float skip_pen, float local_pen,
                              int const *seq, size_t seqlen, int *path);
float map_to_sequence_viterbi_banded(const_scrappie_matrix logpost,
                                     float stay_pen, float skip_pen, float local_pen,
                                     int const *seq, size_t seqlen,
                                     size_t const * poslow, size_t const * poshigh);

// Misc
int * encode_bases_to_integers(char const * seq, size_t n, size_t state_len);
