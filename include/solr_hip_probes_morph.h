/*
 * solr_hip_probes_morph.h - TEST-ONLY entry point of libsolr_hip.so for the key-frame tracks (sol-r_amd/csrc/solr_probes.hip).
 *
 * Like the entry points of solr_hip_probes.h it is not part of the drop-in boundary (include/solr_hip.h) and not used by
 * the product.  solr_hip_probes.h declares the twenty-one probes of the renderer's device functions, of a frame and of the
 * list builders, a set that tests/test_engine_probes_gpu.py holds closed; the probes of the morph kernels are a set of their
 * own, held by tests/test_abi_track.py and used by tests/test_track_gpu.py.
 */
#ifndef SOLR_HIP_PROBES_MORPH_H
#define SOLR_HIP_PROBES_MORPH_H

#include "solr_types.h"

#ifdef __cplusplus
extern "C" {
#endif

/* k_packMorphKeys (solr_morph.hip) as solr_hip_set_morph_track_key launches it, on buffers of the probe's own, with or
 * without a resident scene: key: n primitive records in rank order, rankOf[i]: the record lane i gathers; planes: the seven
 * planes of n float4 each (p0 p1 p2 n0 n1 n2 size; .w is 0).  Runs on solr_hip_get_device().  Returns 0, or -1 with the
 * error set (a null pointer, n < 1, a rank outside 0 ... n - 1 - nothing is launched then -, an error of the runtime's). */
int solr_hip_probe_pack_morph_key(const Primitive *key, const int *rankOf, int n, float *planes);

#ifdef __cplusplus
}
#endif
#endif
