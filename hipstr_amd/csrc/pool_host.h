// pool_host.h — the host twin of the read pooler (pool_host.cpp; plain C++, no HIP): exact pools and median qualities of one locus at a
// time, appended to the caller's arrays, and the assembly of the pooled batch.
#pragma once
#include <stdint.h>
#include <vector>

#include "../../include/hipstr_hmm.h"

struct hipstr_pooled_batch { std::vector<uint8_t> mem; hipstr_batch_t batch; const int32_t* pool_index; };

namespace hipstr_pool {

// Where the next locus' pools go: pools / quals are the entries of the per-pool arrays and the quality bytes written so far.
struct Sink { hipstr_pool_out_t* out; int64_t pools, quals; };

// Locus l of the batch, appended: pool_index of its reads, n_pools[l], pool_off[l] and [l+1], the per-pool arrays from s.pools on, the
// qualities from s.quals on and the offset that closes them.  The caller has checked the tables (validate_tables) and the output arrays.
void pool_locus_host(const hipstr_batch_t* b, int l, Sink& s);
// every locus of the batch
void pool_reads_host(const hipstr_batch_t* b, hipstr_pool_out_t* out);
// the batch ReadPooler leaves behind from a pooling result of b (hipstr_pool_batch); the caller frees it with delete
hipstr_pooled_batch* assemble_pooled_batch(const hipstr_batch_t* b, const hipstr_pool_out_t* o);

}  // namespace hipstr_pool
