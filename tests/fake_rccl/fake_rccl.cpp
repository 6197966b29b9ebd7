// fake_rccl.cpp -- a stand-in transport for the tests of agpt_gather_tiles with world > 1 (tests/test_gpu_fake_rccl_gather.py).
//
// It defines the eight nccl* functions that agpt_comm.hip binds (AGPT_RCCL_FUNCTIONS) for SEVERAL RANKS IN ONE PROCESS ON ONE
// DEVICE, with the HIP runtime API alone: a send is an event recorded on the sender's stream and a note in a mailbox, a receive is a
// wait for that event and a device-to-device copy, both on the receiver's stream.  Nothing here synchronises the host.  The real
// header is included, so every definition below is checked against RCCL's own declaration.  Built by the tests as a shared object
// whose SONAME is librccl.so.1 and loaded by absolute path in a child process before the library under test: that library's
// dlopen("librccl.so.1") is then answered with this object.  One host thread is assumed (the group state is global).
//
// Beside the eight functions: a call log, a one-shot fault hook and a reset (the fake_rccl_* exports at the end).
#include <rccl/rccl.h>

#include <cstdio>
#include <cstring>
#include <deque>
#include <map>
#include <set>
#include <string>
#include <tuple>
#include <vector>

namespace {

struct Comm {
    int world, rank;
    std::string id;   // the 128 bytes
};

struct Op {
    bool send;
    void* buf;
    size_t count;
    ncclDataType_t dtype;
    int peer;
    Comm* comm;
    hipStream_t stream;
};

struct Posted {
    const void* buf;
    size_t count;
    ncclDataType_t dtype;
    hipEvent_t event;
};

using Key = std::tuple<std::string, int, int>;   // (id, source rank, destination rank)

std::set<Comm*> g_comms;
std::vector<Op> g_queue;
std::map<Key, std::deque<Posted>> g_mailbox;
std::vector<std::string> g_log;
int g_depth = 0;
unsigned g_ids = 0;
std::string g_fault_fn;
int g_fault_left = 0;   // calls of g_fault_fn until the one that fails; 0: no fault armed

const char kIdTag[] = "FAKE-RCCL-ID";   // the first bytes of every unique id, the call's number follows

void log_call(const char* fn, int rank, int peer, size_t count, int dtype, const void* stream, ncclResult_t rc) {
    char line[256];
    std::snprintf(line, sizeof line, "%s rank=%d peer=%d count=%zu dtype=%d stream=%p rc=%d depth=%d", fn, rank, peer, count, dtype, stream,
                  (int)rc, g_depth);
    g_log.push_back(line);
}

void log_error(const std::string& what) { g_log.push_back("ERROR " + what); }

// the armed fault: true on the n-th call of fn since it was armed, once
bool fault(const char* fn) {
    if (!g_fault_left || g_fault_fn != fn) return false;
    if (--g_fault_left) return false;
    g_fault_fn.clear();
    return true;
}

size_t size_of(ncclDataType_t t) {
    switch (t) {
        case ncclInt8: case ncclUint8: return 1;
        case ncclFloat16: case ncclBfloat16: return 2;
        case ncclInt32: case ncclUint32: case ncclFloat32: return 4;
        case ncclInt64: case ncclUint64: case ncclFloat64: return 8;
        default: return 0;
    }
}

ncclResult_t enqueue(bool send, const char* fn, const void* buf, size_t count, ncclDataType_t dtype, int peer, ncclComm_t comm, hipStream_t stream) {
    Comm* m = (Comm*)comm;
    const bool known = g_comms.count(m) != 0;
    ncclResult_t rc = ncclSuccess;
    if (fault(fn)) rc = ncclSystemError;
    else if (g_depth == 0) rc = ncclInvalidUsage;
    else if (!known || !buf || !size_of(dtype) || peer < 0 || peer >= m->world || peer == m->rank) rc = ncclInvalidArgument;
    if (rc == ncclSuccess) g_queue.push_back(Op{send, const_cast<void*>(buf), count, dtype, peer, m, stream});
    log_call(fn, known ? m->rank : -1, peer, count, (int)dtype, stream, rc);
    return rc;
}

ncclResult_t execute(const Op& op) {
    char where[96];
    std::snprintf(where, sizeof where, "%s rank=%d peer=%d", op.send ? "Send" : "Recv", op.comm->rank, op.peer);
    if (op.send) {
        hipEvent_t ev = nullptr;
        if (hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess) return log_error(std::string(where) + ": hipEventCreate"), ncclUnhandledCudaError;
        if (hipEventRecord(ev, op.stream) != hipSuccess) {
            (void)hipEventDestroy(ev);
            return log_error(std::string(where) + ": hipEventRecord"), ncclUnhandledCudaError;
        }
        g_mailbox[Key(op.comm->id, op.comm->rank, op.peer)].push_back(Posted{op.buf, op.count, op.dtype, ev});
        return ncclSuccess;
    }
    auto it = g_mailbox.find(Key(op.comm->id, op.peer, op.comm->rank));
    if (it == g_mailbox.end() || it->second.empty()) return log_error(std::string(where) + ": no send was posted"), ncclInternalError;
    const Posted p = it->second.front();
    it->second.pop_front();
    ncclResult_t rc = ncclSuccess;
    if (p.count != op.count || p.dtype != op.dtype) {
        log_error(std::string(where) + ": the sender posted count " + std::to_string(p.count) + " of datatype " + std::to_string((int)p.dtype));
        rc = ncclInvalidArgument;
    } else if (hipStreamWaitEvent(op.stream, p.event, 0) != hipSuccess ||
               (op.count && hipMemcpyAsync(op.buf, p.buf, op.count * size_of(op.dtype), hipMemcpyDeviceToDevice, op.stream) != hipSuccess)) {
        log_error(std::string(where) + ": hipStreamWaitEvent / hipMemcpyAsync");
        rc = ncclUnhandledCudaError;
    }
    (void)hipEventDestroy(p.event);   // (released by the runtime once the wait above has passed it)
    return rc;
}

}  // namespace

extern "C" {

ncclResult_t ncclGetUniqueId(ncclUniqueId* uniqueId) {
    ncclResult_t rc = ncclSuccess;
    if (fault("GetUniqueId")) rc = ncclSystemError;
    else if (!uniqueId) rc = ncclInvalidArgument;
    else {
        static_assert(sizeof(uniqueId->internal) == 128, "the id is 128 bytes");
        const unsigned n = ++g_ids;
        std::memcpy(uniqueId->internal, kIdTag, sizeof kIdTag - 1);
        for (size_t i = sizeof kIdTag - 1; i < sizeof uniqueId->internal; i++) uniqueId->internal[i] = (char)((n * 131u + (unsigned)i * 7u) & 0xFF);
        std::memcpy(uniqueId->internal + sizeof kIdTag - 1, &n, sizeof n);
    }
    log_call("GetUniqueId", -1, -1, 0, -1, nullptr, rc);
    return rc;
}

ncclResult_t ncclCommInitRank(ncclComm_t* comm, int nranks, ncclUniqueId commId, int rank) {
    ncclResult_t rc = ncclSuccess;
    if (fault("CommInitRank")) rc = ncclSystemError;
    else if (!comm || nranks < 1 || rank < 0 || rank >= nranks) rc = ncclInvalidArgument;
    else {
        Comm* m = new Comm{nranks, rank, std::string(commId.internal, sizeof commId.internal)};
        g_comms.insert(m);
        *comm = (ncclComm_t)m;
    }
    log_call("CommInitRank", rank, -1, (size_t)(nranks > 0 ? nranks : 0), -1, nullptr, rc);
    return rc;
}

ncclResult_t ncclCommDestroy(ncclComm_t comm) {
    Comm* m = (Comm*)comm;
    ncclResult_t rc = ncclSuccess;
    int rank = -1;
    if (fault("CommDestroy")) rc = ncclSystemError;
    else if (!g_comms.count(m)) {
        char what[96];
        std::snprintf(what, sizeof what, "CommDestroy: %p is not a live communicator", (void*)comm);
        log_error(what);
        rc = ncclInvalidArgument;
    } else {
        rank = m->rank;
        g_comms.erase(m);
        delete m;
    }
    log_call("CommDestroy", rank, -1, 0, -1, nullptr, rc);
    return rc;
}

ncclResult_t ncclGroupStart() {
    ncclResult_t rc = ncclSuccess;
    if (fault("GroupStart")) rc = ncclSystemError;
    else g_depth++;
    log_call("GroupStart", -1, -1, 0, -1, nullptr, rc);
    return rc;
}

// the outermost end runs what the group queued, in order; the first error is returned and ends the run.  An end that the fault hook
// fails still closes its group, and drops what the group queued.
ncclResult_t ncclGroupEnd() {
    ncclResult_t rc = ncclSuccess;
    if (g_depth == 0) rc = ncclInvalidUsage;
    else {
        g_depth--;
        const bool failed = fault("GroupEnd");
        if (failed) rc = ncclSystemError;
        if (g_depth == 0) {
            std::vector<Op> queue;
            queue.swap(g_queue);
            for (size_t i = 0; i < queue.size() && rc == ncclSuccess; i++) rc = execute(queue[i]);
        }
    }
    log_call("GroupEnd", -1, -1, 0, -1, nullptr, rc);
    return rc;
}

ncclResult_t ncclSend(const void* sendbuff, size_t count, ncclDataType_t datatype, int peer, ncclComm_t comm, hipStream_t stream) {
    return enqueue(true, "Send", sendbuff, count, datatype, peer, comm, stream);
}

ncclResult_t ncclRecv(void* recvbuff, size_t count, ncclDataType_t datatype, int peer, ncclComm_t comm, hipStream_t stream) {
    return enqueue(false, "Recv", recvbuff, count, datatype, peer, comm, stream);
}

const char* ncclGetErrorString(ncclResult_t result) {
    switch (result) {
        case ncclSuccess: return "fake rccl: no error";
        case ncclUnhandledCudaError: return "fake rccl: unhandled HIP error";
        case ncclSystemError: return "fake rccl: unhandled system error";
        case ncclInternalError: return "fake rccl: internal error";
        case ncclInvalidArgument: return "fake rccl: invalid argument";
        case ncclInvalidUsage: return "fake rccl: invalid usage";
        case ncclRemoteError: return "fake rccl: remote error";
        case ncclInProgress: return "fake rccl: operation in progress";
        default: return "fake rccl: unknown result code";
    }
}

// ---- for the tests only -----------------------------------------------------------------------------------------------------------
int fake_rccl_log_count() { return (int)g_log.size(); }

// line i of the log (valid until the next call into this library), NULL past its end
const char* fake_rccl_log_line(int i) { return i >= 0 && (size_t)i < g_log.size() ? g_log[(size_t)i].c_str() : nullptr; }

int fake_rccl_group_depth() { return g_depth; }

int fake_rccl_live_comms() { return (int)g_comms.size(); }

// the n-th call (n >= 1) from now of nccl<function> returns ncclSystemError, once; n = 0 disarms
void fake_rccl_fail_nth(const char* function, int n) {
    g_fault_fn = function && n > 0 ? function : "";
    g_fault_left = function && n > 0 ? n : 0;
}

// Forget the log, the armed fault and every send that no receive has taken (their events are destroyed); returns how many such sends
// there were.  The group depth, the queue of an open group and the live communicators stay: they are what the tests watch.
int fake_rccl_reset() {
    int dropped = 0;
    for (auto& kv : g_mailbox)
        for (const Posted& p : kv.second) {
            (void)hipEventDestroy(p.event);
            dropped++;
        }
    g_mailbox.clear();
    g_log.clear();
    g_fault_fn.clear();
    g_fault_left = 0;
    return dropped;
}

}  // extern "C"
