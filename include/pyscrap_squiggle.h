/* include/pyscrap_squiggle.h -- cdef lines for the squiggle-matching functions scrappy binds (python/pyscrap.h:33-39),
 * with the reference's names and signatures: appended to the cdef text of include/pyscrap_raw.h they route the matching
 * half of scrappy.map_signal_to_squiggle to this library.  The squiggle predictors (pyscrap.h:28-31) are
 * not built here. */

float squiggle_match_viterbi(const raw_table signal, float rate, const_scrappie_matrix params, float prob_back, float local_pen,
                             float skip_pen, float minscore, int32_t *path_padded);
float squiggle_match_forward(const raw_table signal, float rate, const_scrappie_matrix params, float prob_back, float local_pen,
                             float skip_pen, float minscore);
