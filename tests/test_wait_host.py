"""The host's polled wait for a completion word (csrc/bi_wait.h: wait_word) without a GPU: a small stand-alone C++ program with
its own main, compiled against the header with the host compiler, in which a second thread plays the kernel that publishes the
word with a release store.
  1. the word arrives after a short sleep: wait_word returns true and the payload written before the store is visible;
  2. a word that never arrives: false, no earlier than the deadline (with and without a yield phase);
  3. a spin phase as long as the deadline never yields, and still returns.
The program counts the yields itself (sched_yield is a macro for its counter while the header is read)."""
import os
import shutil
import subprocess

import pytest

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'blueice_amd', 'csrc')

PROGRAM = r'''
#include <sched.h>
static int n_yields = 0;
static int counted_yield() { ++n_yields; return ::sched_yield(); }
#define sched_yield counted_yield
#include "bi_wait.h"
#undef sched_yield

#include <cstdio>
#include <thread>

using namespace std::chrono;
static int failures = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } \
    } while (0)

int main() {
    unsigned long long word = 0;
    {   // 1. a publisher: payload, then the word with a release store
        long long payload[8] = {0};
        n_yields = 0;
        std::thread publisher([&] {
            std::this_thread::sleep_for(milliseconds(2));
            for (int i = 0; i < 8; ++i) payload[i] = 1000 + i;
            __atomic_store_n(&word, 7ull, __ATOMIC_RELEASE);
        });
        const bool arrived = wait_word(&word, 7ull, microseconds(30), seconds(10));
        long long sum = 0;
        for (int i = 0; i < 8; ++i) sum += payload[i];
        publisher.join();
        CHECK(arrived);
        CHECK(sum == 8 * 1000 + 28);
        CHECK(n_yields > 0);                        // 2 ms is far beyond the 30 us of spinning
    }
    {   // 2. a word that never arrives: false, and not before the deadline
        n_yields = 0;
        const auto t0 = steady_clock::now();
        const bool arrived = wait_word(&word, 8ull, microseconds(30), milliseconds(20));
        const auto dt = steady_clock::now() - t0;
        CHECK(!arrived);
        CHECK(dt >= milliseconds(20));
        CHECK(dt < seconds(5));
        CHECK(n_yields > 0);
    }
    {   // 3. a spin phase as long as the deadline (the single-point call, the clock every 1024 looks): no yield, and it returns
        n_yields = 0;
        const auto t0 = steady_clock::now();
        const bool arrived = wait_word(&word, 8ull, milliseconds(20), milliseconds(20), 1024);
        const auto dt = steady_clock::now() - t0;
        CHECK(!arrived);
        CHECK(dt >= milliseconds(20));
        CHECK(dt < seconds(5));
        CHECK(n_yields == 0);
        // ... nor when the word is there already or arrives while it spins
        CHECK(wait_word(&word, 7ull, milliseconds(20), milliseconds(20), 1024));
        std::thread publisher([&] {
            std::this_thread::sleep_for(milliseconds(1));
            __atomic_store_n(&word, 9ull, __ATOMIC_RELEASE);
        });
        CHECK(wait_word(&word, 9ull, seconds(10), seconds(10), 1024));
        publisher.join();
        CHECK(n_yields == 0);
    }
    std::printf("%s\n", failures ? "FAILED" : "OK");
    return failures ? 1 : 0;
}
'''


def test_wait_word_program(tmp_path):
    cxx = os.environ.get('CXX') or shutil.which('g++') or shutil.which('c++') or shutil.which('clang++')
    if cxx is None:
        pytest.fail('no host C++ compiler found (CXX, g++, c++, clang++)')
    src = tmp_path / 'wait_word_main.cpp'
    exe = tmp_path / 'wait_word_main'
    src.write_text(PROGRAM)
    build = subprocess.run([cxx, '-O2', '-std=c++17', '-Wall', '-Wextra', '-pthread', '-I', CSRC, '-o', str(exe), str(src)],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    assert build.stderr.strip() == '', build.stderr            # no warnings: the header is plain standard C++ and POSIX
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and run.stdout.strip().endswith('OK'), run.stdout + run.stderr
