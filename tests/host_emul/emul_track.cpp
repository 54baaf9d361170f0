// csrc/k_track.hip compiled for the host (tests/test_track_host_cpu.py).
#include "kernels.h"
#include "k_track.hip"
extern "C" int64_t emul_state_bytes(int slots, int max_dets) { return kasf_sort_stream_bytes(slots, max_dets); }
extern "C" void emul_update(void* state, int B, int slots, int max_dets, const float* dets, int det_rows, int64_t bs, int64_t rs, const int* cnt, int max_age,
                            int min_hits, float thr, int np_, int hold, float* boxes, int* ids, int* slot, int* born, int* count, int* dropped, float* persons, int* pc) {
    kasf_launch_sort_update(nullptr, state, B, slots, max_dets, dets, det_rows, bs, rs, cnt, max_age, min_hits, thr, np_, hold, boxes, ids, slot, born, count, dropped, persons, pc);
}
