// Persistent host worker pools of parallel_for / parallel_io_for (staging
// memcpy, pread / fill callbacks), per device.
#include <condition_variable>

#include "hec_internal.hpp"

namespace hec {

// ---------------------------------------------------------------------------
// Persistent host worker pool (parallel_for). One job at a time: the caller
// publishes it, workers and the caller claim indices from an atomic counter,
// the caller returns when all are done. Workers spin briefly after a job so
// back-to-back small calls find them awake, then sleep on the condition.
// ---------------------------------------------------------------------------
namespace {
class HostPool {
   public:
    // Workers of device `dev`'s pool run on that GPU's NUMA node (when the
    // platform says which; they copy into and out of its pinned staging;
    // profiles/r04/host_pool_bind_ab.jsonl).
    HostPool(unsigned n, int dev) {
        for (unsigned i = 0; i < n; ++i)
            th_.emplace_back([this, dev] {
                (void)hec_bind_thread_to_device(dev, nullptr);  // placement only: no-op when unknown
                loop();
            });
    }
    // false if another caller owns the pool (run serially then)
    bool run(size_t n, unsigned max_threads, const std::function<void(size_t)>& fn) {
        std::unique_lock<std::mutex> own(busy_, std::try_to_lock);
        if (!own.owns_lock()) return false;
        {
            std::lock_guard<std::mutex> lk(mu_);
            fn_ = &fn;
            n_ = n;
            next_.store(0);
            done_.store(0);
            helpers_ = max_threads > 1 ? max_threads - 1 : 0;
            ++gen_;
        }
        cv_.notify_all();
        work();
        while (done_.load(std::memory_order_acquire) < n_) std::this_thread::yield();
        std::lock_guard<std::mutex> lk(mu_);
        fn_ = nullptr;
        // a helper still inside work() has seen next_ >= n_; wait for it to leave
        while (active_.load() != 0) std::this_thread::yield();
        return true;
    }

   private:
    void work() {
        for (;;) {
            const size_t i = next_.fetch_add(1);
            if (i >= n_) return;
            (*fn_)(i);
            done_.fetch_add(1, std::memory_order_release);
        }
    }
    void loop() {
        uint64_t seen = 0;
        for (;;) {
            {
                std::unique_lock<std::mutex> lk(mu_);
                // spin-wait window first (cheap for back-to-back calls), then sleep
                for (int spin = 0; spin < 256 && gen_ == seen; ++spin) {
                    lk.unlock();
                    std::this_thread::yield();
                    lk.lock();
                }
                cv_.wait(lk, [&] { return gen_ != seen; });
                seen = gen_;
                if (!fn_ || helpers_ == 0) continue;
                --helpers_;
                active_.fetch_add(1);
            }
            work();
            active_.fetch_sub(1);
        }
    }
    std::vector<std::thread> th_;
    std::mutex busy_, mu_;
    std::condition_variable cv_;
    const std::function<void(size_t)>* fn_ = nullptr;
    size_t n_ = 0;
    unsigned helpers_ = 0;
    uint64_t gen_ = 0;
    std::atomic<size_t> next_{0}, done_{0};
    std::atomic<int> active_{0};
};
}  // namespace

// Pools per device (up to kPoolsPerDevice each, created on first use and
// never destroyed: their threads live for the process). A call takes a free
// pool of its current device, so the ranges of one multi-device host call --
// and concurrent callers on different GPUs -- copy on their own workers
// instead of all but one running serially. Each pool's workers
// bind themselves to their device's NUMA node, whichever thread created it.
constexpr size_t kPoolsPerDevice = 2;
void pool_run(size_t n, unsigned max_threads, const std::function<void(size_t)>& fn) {
    static std::mutex mu;
    static auto* pools = new std::map<int, std::vector<HostPool*>>();
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) {
        (void)hipGetLastError();
        dev = 0;
    }
    std::vector<HostPool*> mine;
    {
        std::lock_guard<std::mutex> lk(mu);
        mine = (*pools)[dev];
    }
    for (HostPool* p : mine)
        if (p->run(n, max_threads, fn)) return;
    HostPool* fresh = nullptr;
    {
        std::lock_guard<std::mutex> lk(mu);
        auto& v = (*pools)[dev];
        if (v.size() < kPoolsPerDevice) {
            fresh = new HostPool(15, dev);
            v.push_back(fresh);
        }
    }
    if (fresh && fresh->run(n, max_threads, fn)) return;
    for (size_t i = 0; i < n; ++i) fn(i);  // every pool of this device busy: this thread alone
}

}  // namespace hec
