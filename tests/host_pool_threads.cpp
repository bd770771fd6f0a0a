// Host program (no device call) for the process-wide worker pool of ebcc_amd/csrc/host.hpp, the very class the library's
// entropy stage runs on: four caller threads - as four threads of an application inside the library at once - submit batches
// of jobs to HostPool::instance() side by side, each twice with different widths, and check that every job ran exactly once
// and that a throwing job fails its own batch and no other.  Built plain it is a functional test; built with
// -fsanitize=thread it is the data-race check of the pool (tests/test_host_pool_threads.py builds both).
#include <cstdio>

#include "../ebcc_amd/csrc/host.hpp"

using ebcc::HostPool;

int main()
{
    constexpr int kCallers = 4, kRounds = 2;
    constexpr size_t kJobs = 257;
    std::atomic<int> failures{0};
    std::vector<std::thread> callers;
    for (int c = 0; c < kCallers; c++)
        callers.emplace_back([c, &failures]() {
            for (int r = 0; r < kRounds; r++) {
                std::vector<int> ran(kJobs, 0);                          // (job i writes ran[i] alone)
                std::vector<unsigned long long> sum(kJobs, 0);
                const bool thrower = c == 1 && r == 1;
                auto batch = HostPool::instance().submit(kJobs, 2 + (unsigned) (c + r) % 3, [&](size_t i) {
                    ran[i]++;
                    for (unsigned k = 0; k < 2000; k++) sum[i] += (i + 1) * k;
                    if (thrower && i == 100) throw std::runtime_error("job 100");
                });
                const bool ok = batch->wait();
                if (ok == thrower) { std::printf("caller %d round %d: wait() returned %d\n", c, r, (int) ok); failures++; }
                if (thrower && batch->error != "job 100") { std::printf("caller %d: error text '%s'\n", c, batch->error.c_str()); failures++; }
                for (size_t i = 0; i < kJobs; i++)
                    if (ran[i] != 1 || sum[i] != (i + 1) * 1999000ull) { std::printf("caller %d round %d job %zu: ran %d times\n", c, r, i, ran[i]); failures++; break; }
            }
        });
    for (auto &t : callers) t.join();
    const unsigned workers = HostPool::instance().threads();
    if (workers < 1 || workers > 4) { std::printf("%u workers for widths of 2 to 4\n", workers); failures++; }
    std::printf("%d failures, %u workers\n", failures.load(), workers);
    return failures.load() ? 1 : 0;
}
