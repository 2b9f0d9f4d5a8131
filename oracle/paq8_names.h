/* oracle/paq8_names.h -- TEST INFRASTRUCTURE ONLY (force-included by the Makefile into the product's parser files that the oracle
 * also builds: cmix_amd/csrc/p8front/p8f_{stem,text,word,xml,record,exe}.c).
 * Those files are byte-stream state machines with no learner of their own. In the product their contexts go to the emitter of the chunk
 * being built (p8f_emit.c) and the device learns; here the same calls reach the oracle's CPU learners (paq8_core.c, paq8_maps.c), and
 * the entry points keep the names oracle.py and the tests bind. One #define per name. */
#ifndef ORACLE_PAQ8_NAMES_H
#define ORACLE_PAQ8_NAMES_H
#include "orc_alloc.h"
/* the backend the parsers call */
#define p8f_tracked_calloc orc_t_calloc
#define p8f_hash2 orc_p8_hash2
#define p8f_hash3 orc_p8_hash3
#define p8f_hash4 orc_p8_hash4
#define p8f_hash5 orc_p8_hash5
#define p8f_combine64 orc_p8_combine64
#define p8f_finalize64 orc_p8_finalize64
#define p8f_ilog orc_p8_ilog
#define p8f_cm_new orc_p8_cm_new
#define p8f_cm_step orc_p8_cm_step
#define p8f_cm2_new orc_p8_cm2_new
#define p8f_cm2_step orc_p8_cm2_step
#define p8f_dmap_new orc_p8_dmap_new
#define p8f_dmap_mix orc_p8_dmap_mix
#define p8f_dmap_set_direct orc_p8_dmap_set_direct
/* the entry points the oracle's predictor and its Python bindings use */
#define p8f_stem_word orc_p8_stem_word
#define p8f_en_stem_word orc_p8_en_stem_word
#define p8f_text_new orc_p8_text_new
#define p8f_text_step orc_p8_text_step
#define p8f_word_new orc_p8_word_new
#define p8f_word_step orc_p8_word_step
#define p8f_xml_new orc_p8_xml_new
#define p8f_xml_step orc_p8_xml_step
#define p8f_record_new orc_p8_record_new
#define p8f_record_step orc_p8_record_step
#define p8f_exe_new orc_p8_exe_new
#define p8f_exe_step orc_p8_exe_step
#define p8f_exe_debug orc_p8_exe_debug
#endif
