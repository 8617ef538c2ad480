// sched_selftest.cpp -- the emulator's scheduler checked on kernels of its own (test infrastructure only; built and run by
// tests/test_emu_schedule.py with hip_emu.cpp, under the schedules of ZMI_EMU_SCHED).
//   order     after a barrier and after every rendezvous the lanes of a wave resume in lane order: 64 lanes store their number to one
//             LDS cell, the highest lane's stays (what lz77.hip's 16-bit hash heads lean on).  Prints the cells read back.
//   flag      a wave spins on an LDS flag another wave sets after some exchanges of its own: ends, prints the value passed.
//   deadlock  half a wave waits in a wave exchange, everybody else at the barrier: the DEADLOCK report, abort.
//   livelock  a wave spins on a flag nobody sets: the LIVELOCK report, abort.
#include "hip_emu.h"
#include <string>

static void k_order(int* out) {
    int* cell = (int*)emu::g.dyn_smem;
    const unsigned w = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    __syncthreads();
    for (int r = 0; r < 3; ++r) {
        cell[w] = (int)lane + 100 * r;
        emu::wave_rendezvous(0, false);
        if (lane == 0) out[(blockIdx.x * 2 + w) * 3 + r] = cell[w];
        emu::wave_rendezvous(0, false);
    }
}

static void k_flag(int* out) {
    volatile int* flag = (volatile int*)emu::g.dyn_smem;
    const unsigned w = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    if (threadIdx.x == 0) flag[0] = 0;
    __syncthreads();
    if (w == 0) {
        int v = (int)lane;
        for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);   // 2016 in every lane
        if (lane == 0) flag[0] = v;
    } else {
        while (flag[0] == 0) emu::spin_yield();
        if (lane == 0) out[blockIdx.x] = flag[0];
    }
}

static void k_deadlock() {
    if (threadIdx.x < 32u) emu::wave_rendezvous(0, false);
    else __syncthreads();
}

static void k_livelock() {
    volatile int* flag = (volatile int*)emu::g.dyn_smem;
    if (threadIdx.x == 0) flag[0] = 0;
    __syncthreads();
    if (threadIdx.x < 64u) while (flag[0] == 0) emu::spin_yield();
}

int main(int argc, char** argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    int out[12] = {0};
    if (mode == "order") {
        emu::launch(dim3(2), dim3(128), 64, [&]() { k_order(out); });
        for (int i = 0; i < 12; ++i) printf("%d%c", out[i], i == 11 ? '\n' : ' ');
    } else if (mode == "flag") {
        emu::launch(dim3(2), dim3(128), 64, [&]() { k_flag(out); });
        printf("%d %d\n", out[0], out[1]);
    } else if (mode == "deadlock") {
        emu::launch(dim3(1), dim3(128), 64, []() { k_deadlock(); });
    } else if (mode == "livelock") {
        emu::launch(dim3(1), dim3(128), 64, []() { k_livelock(); });
    } else {
        fprintf(stderr, "usage: sched_selftest order|flag|deadlock|livelock\n");
        return 2;
    }
    return 0;
}
