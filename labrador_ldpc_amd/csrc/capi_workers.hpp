// capi_workers.hpp -- part of capi.hip: the persistent per-device worker threads, the device set of a call and sharding.
#pragma once

namespace {

// ---- host batches over several GPUs -------------------------------------------------------------------
// Frames are independent (src/lib.rs:15-17), so a host batch splits into contiguous slices, one per
// listed device, each run through that device's own host pipeline by a worker thread of this library
// -- the shape of the reference's harness, one worker per core over independent frames
// (perftest/src/main.rs:39-45), with GPUs for cores.  No data crosses between devices; the only
// aggregation is the status.  Workers are persistent (their per-thread staging buffers, streams and
// pinned memory survive between calls) and never destroyed: at process exit they are parked on their
// condition variable.
void shard_range(size_t total, size_t parts, size_t index, size_t *first, size_t *count)
{
    const size_t base = total / parts, extra = total % parts;
    *first = index * base + (index < extra ? index : extra);
    *count = base + (index < extra ? 1 : 0);
}

// NUMA placement of a device's worker (round 2's review, weak #7): the host path is bound by PCIe at ~55 GB/s per GPU, and
// eight of them read ~440 GB/s of host memory -- more than one socket's interconnect carries if every staging copy starts on
// the wrong node.  A worker pins itself to the CPUs local to its GPU (sysfs: /sys/bus/pci/devices/<bus id>/local_cpulist,
// intersected with the CPUs the process may use) BEFORE it allocates anything, so its pinned staging memory is first touched
// on that node and its pageable copies run there; its collector thread inherits the mask.  Best effort: any failure (no sysfs
// entry, an empty intersection, LABRADOR_LDPC_HIP_NO_NUMA set) leaves the thread where it is.
void pin_to_device_node(int dev)
{
    if (ldpc::env_flag("LABRADOR_LDPC_HIP_NO_NUMA")) return;
    char bus[32] = {};
    if (hipDeviceGetPCIBusId(bus, (int)sizeof bus, dev) != hipSuccess) { (void)hipGetLastError(); return; }
    for (char *c = bus; *c; ++c) if (*c >= 'A' && *c <= 'F') *c = (char)(*c - 'A' + 'a');       // sysfs spells hex digits in lower case
    char path[128];
    std::snprintf(path, sizeof path, "/sys/bus/pci/devices/%s/local_cpulist", bus);
    FILE *f = std::fopen(path, "r");
    if (!f) return;
    char list[4096] = {};
    const bool got = std::fgets(list, (int)sizeof list, f) != nullptr;
    std::fclose(f);
    if (!got) return;
    cpu_set_t allowed, want;
    CPU_ZERO(&allowed); CPU_ZERO(&want);
    if (sched_getaffinity(0, sizeof allowed, &allowed) != 0) return;
    int n = 0;
    for (const char *p = list; *p && *p != '\n';) {                                              // "0-23,96-119"
        char *end = nullptr;
        long a = std::strtol(p, &end, 10), b = a;
        if (end == p) break;
        if (*end == '-') { p = end + 1; b = std::strtol(p, &end, 10); }
        for (long c = a; c <= b && c < CPU_SETSIZE; ++c)
            if (c >= 0 && CPU_ISSET((int)c, &allowed)) { CPU_SET((int)c, &want); ++n; }
        p = (*end == ',') ? end + 1 : end;
        if (*end != ',' ) break;
    }
    if (n > 0) (void)sched_setaffinity(0, sizeof want, &want);
}

struct Worker {
    struct Job {
        std::function<int()> fn;
        int status = LABRADOR_LDPC_HIP_OK;
        std::string err;
        bool done = false;
    };
    std::mutex m;
    std::condition_variable cv;
    std::deque<Job *> queue;
    const int dev;                                     // the one device this worker ever serves
    explicit Worker(int device) : dev(device) { std::thread([this] { run(); }).detach(); }
    void run()
    {
        pin_to_device_node(dev);
        for (;;) {
            Job *j = nullptr;
            {
                std::unique_lock<std::mutex> lk(m);
                cv.wait(lk, [&] { return !queue.empty(); });
                j = queue.front();
                queue.pop_front();
            }
            g_err.clear();
            const int st = j->fn();
            {
                std::lock_guard<std::mutex> lk(m);
                j->status = st;
                j->err = g_err;
                j->done = true;
            }
            cv.notify_all();
        }
    }
    void post(Job *j)
    {
        { std::lock_guard<std::mutex> lk(m); queue.push_back(j); }
        cv.notify_all();
    }
    void wait(Job *j)
    {
        std::unique_lock<std::mutex> lk(m);
        cv.wait(lk, [&] { return j->done; });
    }
};

// Workers are keyed by (device ordinal, how many times that ordinal has occurred in the list so far): a worker's
// thread-local staging pool, streams and pinned buffer hold ONE device's resources, so it must keep serving that device
// whatever order a later call lists the devices in (by position, [0, 1] followed by [1, 0] made every worker free and
// re-create everything).  The detached threads do not survive fork(): the child gets a fresh, empty pool (atfork handler;
// the parent's Worker objects are leaked in the child on purpose -- their mutexes may be held by threads that no longer
// exist), and its first sharded call starts its own workers.
struct WorkerPool {
    std::mutex m;
    std::vector<std::vector<Worker *>> by_dev;         // [device][occurrence]
};
WorkerPool *g_workers = new WorkerPool;                // leaked on purpose: workers are parked on their condition variable at exit
void workers_after_fork_in_child() { g_workers = new WorkerPool; }

// At most this many workers (threads, each with its own streams, events and staging) per device: further repeats of an ordinal in
// one call queue behind them -- a worker's queue serialises its jobs -- so a call with hundreds of parts on one GPU leaves four
// threads behind, not hundreds (round 5 advice).  Four pipelines already saturate a GPU's copy engines and its kernel slot.
constexpr size_t MAX_WORKERS_PER_DEVICE = 4;

Worker &worker(int dev, size_t occurrence)
{
    occurrence %= MAX_WORKERS_PER_DEVICE;
    static const int registered = pthread_atfork(nullptr, nullptr, workers_after_fork_in_child);
    (void)registered;
    WorkerPool &p = *g_workers;
    std::lock_guard<std::mutex> lk(p.m);
    if (p.by_dev.size() <= (size_t)dev) p.by_dev.resize((size_t)dev + 1);
    auto &v = p.by_dev[(size_t)dev];
    while (v.size() <= occurrence) v.push_back(new Worker(dev));
    return *v[occurrence];
}

// The devices a call should shard over: empty = single-device call.  Returns a status.
int device_set(const labrador_ldpc_hip_opts *opts, std::vector<int> &devs)
{
    devs.clear();
    if (!opts) return LABRADOR_LDPC_HIP_OK;
    const bool list = opts->n_devices > 0;
    if (!list && opts->device != LABRADOR_LDPC_HIP_DEVICE_ALL) {
        if (opts->n_devices < 0) return fail(LABRADOR_LDPC_HIP_EINVAL, "opts->n_devices is negative");
        if (opts->device < LABRADOR_LDPC_HIP_DEVICE_ALL) return fail(LABRADOR_LDPC_HIP_EINVAL, "bad opts->device %d", opts->device);
        return LABRADOR_LDPC_HIP_OK;
    }
    if (opts->memory != LABRADOR_LDPC_HIP_MEM_HOST)
        return fail(LABRADOR_LDPC_HIP_EINVAL, "a device set needs MEM_HOST buffers (device memory lives on one device)");
    if (opts->stream) return fail(LABRADOR_LDPC_HIP_EINVAL, "a device set runs on the library's own streams; opts->stream must be NULL");
    int count = 0;
    if (int s = device_count_or_fail(&count)) return s;
    if (list) {
        if (!opts->devices) return fail(LABRADOR_LDPC_HIP_EINVAL, "opts->n_devices > 0 but opts->devices is NULL");
        if (opts->n_devices > 1024) return fail(LABRADOR_LDPC_HIP_EINVAL, "opts->n_devices too large");
        for (int i = 0; i < opts->n_devices; ++i) {
            const int d = opts->devices[i];
            if (d < 0 || d >= count) return fail(LABRADOR_LDPC_HIP_EINVAL, "devices[%d] = %d out of range (%d devices)", i, d, count);
            if (!device_is_gfx950(d)) return fail(LABRADOR_LDPC_HIP_ENODEV, "device %d is not gfx950", d);
            devs.push_back(d);
        }
    } else {
        for (int d = 0; d < count; ++d)
            if (device_is_gfx950(d)) devs.push_back(d);
        if (devs.empty()) return fail(LABRADOR_LDPC_HIP_ENODEV, "no gfx950 device; this library carries gfx950 code only");
    }
    return LABRADOR_LDPC_HIP_OK;
}

// The one loop that hands the parts of a call to the device workers and collects them.  make_job(i) is part i's job, or an empty
// function for a part with nothing to run: such a part is not posted and is no occurrence of its device.  Part i runs on the worker
// of (dev_of(i), how many posted parts before it have that device).  The status is the first failing part's, the error its text
// behind prefix(i, buffer, size).
// Starting a worker or queueing a job can throw (std::thread, bad_alloc).  Jobs already posted hold pointers into `jobs`: they
// are waited for below before this frame unwinds, and no exception crosses the C ABI.
template <class DevOf, class MakeJob, class Prefix>
int post_and_wait(size_t parts, DevOf dev_of, MakeJob make_job, Prefix prefix)
{
    std::vector<Worker::Job> jobs(parts);
    std::vector<Worker *> who(parts, nullptr);
    int status = LABRADOR_LDPC_HIP_OK;
    try {
        for (size_t i = 0; i < parts; ++i) {
            jobs[i].fn = make_job(i);
            if (!jobs[i].fn) continue;
            size_t occurrence = 0;
            for (size_t k = 0; k < i; ++k) occurrence += (who[k] && dev_of(k) == dev_of(i)) ? 1 : 0;
            Worker *w = &worker(dev_of(i), occurrence);
            w->post(&jobs[i]);
            who[i] = w;                                  // set only once the job is queued
        }
    } catch (const std::exception &e) {
        status = fail(LABRADOR_LDPC_HIP_ERUNTIME, "could not start the device workers: %s", e.what());
    }
    for (size_t i = 0; i < parts; ++i) {
        if (!who[i]) continue;
        who[i]->wait(&jobs[i]);
        if (jobs[i].status != LABRADOR_LDPC_HIP_OK && status == LABRADOR_LDPC_HIP_OK) {
            status = jobs[i].status;
            char pre[64];
            prefix(i, pre, sizeof pre);
            g_err = pre + jobs[i].err;
        }
    }
    return status;
}

// run(first_item, n_items, opts_for_one_device) -> status, once per device on that device's worker
template <class Run>
int run_sharded(const std::vector<int> &devs, size_t items, int variant, Run run)
{
    const size_t parts = devs.size();
    std::vector<labrador_ldpc_hip_opts> sub(parts);
    for (size_t i = 0; i < parts; ++i)
        sub[i] = labrador_ldpc_hip_opts{sizeof(labrador_ldpc_hip_opts), devs[i], LABRADOR_LDPC_HIP_MEM_HOST, nullptr, variant, 0, nullptr};
    return post_and_wait(
        parts, [&](size_t i) { return devs[i]; },
        [&](size_t i) -> std::function<int()> {
            size_t first, count;
            shard_range(items, parts, i, &first, &count);
            const labrador_ldpc_hip_opts *o = &sub[i];
            return [=]() -> int { return count ? run(first, count, o) : LABRADOR_LDPC_HIP_OK; };
        },
        [&](size_t i, char *pre, size_t cap) { std::snprintf(pre, cap, "device %d: ", devs[i]); });
}

}  // namespace
