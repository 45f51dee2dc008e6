/* include/pyscrap_events.h -- the cdef line for event detection as scrappy binds it (python/pyscrap.h:65), with the reference's name
 * and signature: appended to the cdef text of include/pyscrap_raw.h it routes scrappy's event-detection helper to this library
 * (`detector_param` is in the struct block build.py already has).  A read without a peak gives .event == NULL. */

event_table detect_events(raw_table const rt, detector_param const edparam);
