// What plonkprove.hip (one proof a call) shares with plonkprove_many.hip (m proofs a call): the
// object, a refusal that carries its status, and the lone proof's core, which the many-call loops over at a chunk width of 1.
#pragma once
#include "plonk_internal.hpp"
#include "plonk_transcript.hpp"
#include "plonk_many_plan.hpp"

constexpr uint32_t PLONK_ROUNDS = 5;

struct PlonkMany;                                     // plonkprove_many.hip: the table, the slots and the batched multiplication's buffers
void plonk_many_free(PlonkMany *m);
size_t plonk_many_bytes(const PlonkMany *m);          // 0 for null: nothing was made

struct zk_plonk_prover {
    zk_kzg *kzg = nullptr;                            // borrowed: it outlives the object
    zk_plonk_r1cs *r1cs = nullptr;                    // borrowed too: the compiled circuit of a prover made by zk_plonk_prover_create_r1cs
    int device = 0;
    uint32_t log_n = 0;
    uint64_t n = 0, cap = 0, n_witness = 0, n_public = 0;
    std::mutex mu;                                    // calls on one object are serialised
    std::unique_ptr<Stream> st;
    zk_plonk_circuit *circ = nullptr;                 // round 3's extensions and work vectors: owned
    zk_plonk_opening *open = nullptr;                 // rounds 4 and 5's coefficients and a proof's rows: owned
    PlonkPerm *perm = nullptr;                        // round 2's work buffers: owned
    PlonkMany *many = nullptr;                        // made by the first many-call that needs it: owned
    DevBuf<uint32_t> maps;                            // 3 x n
    DevBuf<Fr> sig, shifts;                           // s1 .. s3 by values, 3 x n; 1, k1, k2
    DevBuf<Fr> wit, pub, blind;                       // a call's witness, publics and blinds
    DevBuf<Fr> vals;                                  // 4 x n: a, b, c and PI by values
    DevBuf<Fr> zval, pic;                             // z by values; PI by coefficients
    zk_plonk_vkey vk;
    uint32_t last_launches = 0, round_launches[PLONK_ROUNDS] = {0, 0, 0, 0, 0};
    struct {                                          // of the last many-call (zk_plonk_prover_many_info)
        uint32_t chunks = 0, multiplications = 0, launches = 0, drains = 0, refused = 0;
    } many_last;
    size_t own_bytes() const {
        return maps.bytes() + sig.bytes() + shifts.bytes() + wit.bytes() + pub.bytes() + blind.bytes() + vals.bytes() + zval.bytes() + pic.bytes();
    }
    ~zk_plonk_prover() {
        if (many) plonk_many_free(many);
        if (perm) plonk_perm_free(perm);
        if (open) zk_plonk_opening_destroy(open);
        if (circ) zk_plonk_circuit_destroy(circ);
    }
};

// A witness the prover refuses: an error of zk_plonk_prove as before (what() is the text it always was), a status to the many-call
struct PlonkRefusal : std::invalid_argument {
    uint32_t status;
    PlonkRefusal(uint32_t status_, const std::string &text) : std::invalid_argument(text), status(status_) {}
};

// plonkprove.hip's five rounds over what is resident in p->wit, p->pub and p->blind (the caller holds p->mu and the device and
// has queued their copies on the stream); publics: the host's copy, for the transcript; first: the launch counter where the
// call began.  Throws PlonkRefusal for a bad witness, and then no proof byte is written
void plonk_prover_core(zk_plonk_prover *p, const char *who, uint8_t *proof, const uint8_t *publics, uint32_t seg, uint64_t first);
