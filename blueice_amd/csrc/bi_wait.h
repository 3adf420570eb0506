// bi_wait.h -- the host's polled wait for a completion word that a kernel publishes in pinned host memory with a system-scope
// release store (k_morph_single, k_plan_report, publish_when_last of the toy-MC finish kernels).  Standard and POSIX headers
// only: a CPU program can compile it (tests/test_wait_host.py).
#pragma once

#include <sched.h>

#include <chrono>

// Wait until *word == seq: busy for the first `spin` (a yield costs more than a short wait is worth), then giving the core away
// between looks -- eight ranks of a node each burning a core per call is what the launcher's thread cap exists to prevent --
// until `deadline` (both from now).  spin >= deadline: no yield phase.  The spin phase looks at the clock every `look_every`
// spins (a power of two).  Returns whether the word arrived; what the publisher wrote before its release store is then
// visible (every look is an acquire load: a plain load on x86).  A caller whose word never came falls back to
// hipStreamSynchronize, which also reports a faulted kernel.
inline bool wait_word(const volatile unsigned long long* word, unsigned long long seq, std::chrono::microseconds spin,
                      std::chrono::microseconds deadline, unsigned look_every = 64) {
    const auto t_start = std::chrono::steady_clock::now();
    const auto t_spin = t_start + spin, t_end = t_start + deadline;
    bool arrived = false, yielding = false;
    for (unsigned n = 0; !(arrived = (__atomic_load_n(word, __ATOMIC_ACQUIRE) == seq)); ++n) {
        if (yielding) {
            sched_yield();
            if (std::chrono::steady_clock::now() > t_end) break;
            continue;
        }
#if defined(__x86_64__) || defined(__i386__)
        __builtin_ia32_pause();
#endif
        if ((n & (look_every - 1)) != look_every - 1) continue;
        const auto now = std::chrono::steady_clock::now();
        if (now > t_end) break;
        if (now > t_spin) yielding = true;
    }
    return arrived;
}
