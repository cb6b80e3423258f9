// inflate_batch_dict.hip -- k_inflate_batch<true>: the batch decoder for streams made with a
// preset dictionary (dmx_inflate_batch_dict_device), compiled apart from the plain kernel (see
// inflate_batch.hip).
#define DMX_BATCH_DICT 1
#include "inflate_batch.hip"
