/* include/pyscrap_squiggle_net.h -- cdef lines for the squiggle predictors scrappy binds (python/pyscrap.h:29-31), with the
 * reference's names and signatures: appended to the cdef text of include/pyscrap_raw.h and include/pyscrap_squiggle.h they
 * route scrappy.sequence_to_squiggle and the predicting half of scrappy.map_signal_to_squiggle to this library
 * (INTEGRATION.md).  The weights are data: register a .scrm under each name before the first call. */

scrappie_matrix squiggle_r94(int const * sequence, size_t n, bool transform_units);
scrappie_matrix squiggle_r94_rna(int const * sequence, size_t n, bool transform_units);
scrappie_matrix squiggle_r10(int const * sequence, size_t n, bool transform_units);
