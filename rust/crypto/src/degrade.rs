//! What the drop-in does when the MI355X engine cannot answer at all.
//!
//! The engine already recovers from device faults on its own: a failed shard
//! or queue window is re-run on a rebuilt context, then on every other
//! context of every GPU (`coa_engine_recoveries`, `coa_queue_metrics`'
//! retried / recovered counters).  Only when every attempt failed -- or no
//! GPU was ever found -- does a call return a negative status.  The
//! reference's `Signature::verify` cannot fail for any reason but the
//! signature (crypto/src/lib.rs:200-219), and `Core::run` logs every error
//! and carries on (primary/src/core.rs:390-398), so an engine failure must
//! never become a verdict ("verdicts never depend on device
//! health").
//!
//! Policy, chosen by `COA_ON_ENGINE_FAILURE` (read once per process):
//!   * `cpu` (the default) -- the call is answered by the ENGINE'S OWN CPU
//!     path, `coa_cpu_*` in include/coa_verify.h (csrc/coa_cpu.cpp: the same
//!     dalek 1.0.1 acceptance rules as the GPU kernels, radix-2^51 field
//!     arithmetic and Straus windows on the host's cores, checked against the
//!     golden fixtures and the test oracle by tests/test_cpu_path.py).  It is
//!     neither ed25519-dalek (the replaced implementation) nor the test
//!     oracle (oracle/, never linked into the product).  Each degraded call
//!     is counted (`degraded_calls`) and the first ones are reported on
//!     stderr with the engine's status, so a node running on its CPU is
//!     visible rather than silently slow.
//!   * `panic` -- the caller panics with the engine's message (for
//!     deployments that would rather restart a node than run it at CPU
//!     speed).
//!
//! Wiring: `pub mod degrade;` in crypto/src/lib.rs, used by gpu.rs,
//! service.rs and the primary's gpu_certificate.rs.
use crate::coa_ffi as ffi;
use crate::{CryptoError, Digest, PublicKey};
use std::sync::atomic::{AtomicU64, AtomicU8, Ordering};

static DEGRADED: AtomicU64 = AtomicU64::new(0);
/// 0 = not read yet, 1 = cpu, 2 = panic
static POLICY: AtomicU8 = AtomicU8::new(0);
/// Degraded calls reported on stderr before going quiet (the counter keeps
/// counting).
const REPORTED: u64 = 16;
/// Host threads of the CPU path (0 = min(16, hardware threads)).
const CPU_THREADS: i32 = 0;

fn panics() -> bool {
    let mut p = POLICY.load(Ordering::Relaxed);
    if p == 0 {
        p = match std::env::var("COA_ON_ENGINE_FAILURE") {
            Ok(v) if v == "panic" => 2,
            _ => 1,
        };
        POLICY.store(p, Ordering::Relaxed);
    }
    p == 2
}

/// An engine call of kind `what` returned status `rc` < 0 (message `msg`):
/// panics under the `panic` policy, otherwise counts and reports the call
/// once (a window of many certificates is one call), which the caller then
/// answers with the engine's CPU path.
pub fn engine_failed(rc: i32, msg: &str, what: &str) {
    if panics() {
        panic!("MI355X verification engine failure {} in {}: {}", rc, what, msg);
    }
    let n = DEGRADED.fetch_add(1, Ordering::Relaxed) + 1;
    if n <= REPORTED {
        eprintln!(
            "MI355X verification engine failure {} in {} ({}): answered by the engine's CPU path (degraded call #{}{})",
            rc,
            what,
            msg,
            n,
            if n == REPORTED { "; further ones are counted, not reported" } else { "" }
        );
    }
}

/// Calls answered on the CPU since the process started.
pub fn degraded_calls() -> u64 {
    DEGRADED.load(Ordering::Relaxed)
}

/// The CPU path answers every well-formed call; a negative status here means
/// the arguments themselves were malformed, which no verdict can paper over.
fn cpu_status(rc: i32, what: &str) -> i32 {
    assert!(rc >= 0, "engine CPU path refused {}: status {}", what, rc);
    rc
}

fn result_of(v: i32) -> Result<(), CryptoError> {
    if v == 0 {
        Ok(())
    } else {
        Err(CryptoError::new())
    }
}

/// `Signature::verify` (crypto/src/lib.rs:200-204) on the engine's CPU path.
pub fn cpu_verify(signature: &[u8; 64], digest: &Digest, public_key: &PublicKey) -> Result<(), CryptoError> {
    let rc = unsafe {
        ffi::coa_cpu_ed25519_verify_strict(digest.0.as_ptr(), 32, public_key.0.as_ptr(), signature.as_ptr())
    };
    result_of(cpu_status(rc, "Signature::verify"))
}

/// `Signature::verify_batch` (crypto/src/lib.rs:206-219) on the engine's CPU
/// path, weights from OS entropy (rng_seed 0) as dalek's thread_rng.
pub fn cpu_verify_batch(digest: &Digest, votes: &[(PublicKey, [u8; 64])]) -> Result<(), CryptoError> {
    let (mut pks, mut sigs) = (Vec::with_capacity(32 * votes.len()), Vec::with_capacity(64 * votes.len()));
    for (key, sig) in votes {
        pks.extend_from_slice(&key.0);
        sigs.extend_from_slice(sig);
    }
    let rc = unsafe {
        ffi::coa_cpu_ed25519_verify_batch(digest.0.as_ptr(), pks.as_ptr(), sigs.as_ptr(), votes.len(), 0)
    };
    result_of(cpu_status(rc, "Signature::verify_batch"))
}

/// `Digest(Sha512(bytes)[..32])` (worker/src/processor.rs:38) on the CPU path.
pub fn cpu_digest(bytes: &[u8]) -> Digest {
    let offsets = [0u64, bytes.len() as u64];
    let mut out = [0u8; 64];
    let rc = unsafe { ffi::coa_cpu_sha512_many(bytes.as_ptr(), offsets.as_ptr(), 1, out.as_mut_ptr(), 1) };
    cpu_status(rc, "Digest");
    let mut d = [0u8; 32];
    d.copy_from_slice(&out[..32]);
    Digest(d)
}

/// The COA_CERT_BAD_HEADER_ID / COA_CERT_BAD_HEADER_SIG bits of
/// `Header::verify`'s two crypto checks (primary/src/messages.rs:49-51,
/// 64-66) for many headers on the engine's CPU path.  Arrays as
/// `coa_header_verify_many` takes them: concatenated digest inputs with
/// n + 1 offsets, 32-byte ids and authors, 64-byte signatures.
pub fn cpu_header_bits(header_data: &[u8], header_offsets: &[u64], ids: &[u8], authors: &[u8], sigs: &[u8]) -> Vec<u8> {
    let n = ids.len() / 32;
    assert!(header_offsets.len() == n + 1 && authors.len() == 32 * n && sigs.len() == 64 * n);
    let mut status = vec![0xffu8; n];
    let rc = unsafe {
        ffi::coa_cpu_header_verify_many(header_data.as_ptr(), header_offsets.as_ptr(), ids.as_ptr(), authors.as_ptr(),
                                        sigs.as_ptr(), n, status.as_mut_ptr(), CPU_THREADS)
    };
    cpu_status(rc, "Header::verify (many)");
    status
}

/// `Vote::verify`'s signature check (primary/src/messages.rs:139-141 over
/// `Vote::digest`, :145-153) for many votes on the engine's CPU path: one
/// verdict byte per vote, 0 Ok / 1 Err.
pub fn cpu_vote_verdicts(ids: &[u8], rounds: &[u64], origins: &[u8], authors: &[u8], sigs: &[u8]) -> Vec<u8> {
    let n = rounds.len();
    assert!(ids.len() == 32 * n && origins.len() == 32 * n && authors.len() == 32 * n && sigs.len() == 64 * n);
    let mut verdicts = vec![1u8; n];
    let rc = unsafe {
        ffi::coa_cpu_vote_verify_many(ids.as_ptr(), rounds.as_ptr(), origins.as_ptr(), authors.as_ptr(), sigs.as_ptr(),
                                      n, verdicts.as_mut_ptr(), CPU_THREADS)
    };
    cpu_status(rc, "Vote::verify (many)");
    verdicts
}

/// The COA_CERT_* bits of `Certificate::verify`'s three crypto checks
/// (primary/src/messages.rs:48-67,189-215), each evaluated on its own as the
/// engine reports them: bit 0 `Header::digest != id` (:70-84), bit 1 the
/// header's `Signature::verify(id, author)` (:64-66), bit 2
/// `Signature::verify_batch(Certificate::digest, votes)` (:214, digest
/// :226-233).  Inputs as the engine takes them: the header's digest input,
/// id, origin, header signature, round and the votes' concatenated 32-byte
/// keys and 64-byte signatures.
pub fn cpu_certificate_bits(header_input: &[u8], id: &[u8], origin: &[u8], header_signature: &[u8], round: u64,
                            vote_keys: &[u8], vote_signatures: &[u8]) -> u8 {
    assert!(id.len() == 32 && origin.len() == 32 && header_signature.len() == 64);
    let hoff = [0u64, header_input.len() as u64];
    let voff = [0u64, (vote_keys.len() / 32) as u64];
    let mut status = [0xffu8; 1];
    let rc = unsafe {
        ffi::coa_cpu_certificate_verify_many(header_input.as_ptr(), hoff.as_ptr(), id.as_ptr(), origin.as_ptr(),
                                             header_signature.as_ptr(), &round, vote_keys.as_ptr(),
                                             vote_signatures.as_ptr(), voff.as_ptr(), 1, 0, status.as_mut_ptr(),
                                             CPU_THREADS)
    };
    cpu_status(rc, "Certificate::verify");
    status[0]
}

/// `config::Committee` as the arrays `coa_committee_register_authorities` and
/// the stateless `coa_cpu_*_verdict_many` calls take: authority i has key
/// `keys[32 i ..]`, stake `stakes[i]` and the worker ids
/// `worker_ids[worker_offsets[i] .. worker_offsets[i + 1])`.
pub struct CommitteeArrays {
    pub keys: Vec<u8>,
    pub stakes: Vec<u32>,
    pub worker_ids: Vec<u32>,
    pub worker_offsets: Vec<u64>,
}

/// "dispatch, then verify" (primary/src/primary.rs:223-244, then
/// primary/src/messages.rs:48-67, 131-142, 189-215) for a receive buffer of
/// interleaved frames on the engine's CPU path: per frame its kind and its
/// COA_DAG_* word, COA_DAG_NO_MESSAGE where the reference drops the frame.
/// `frames` is the buffer, frame i its bytes `offsets[i] .. offsets[i + 1]`.
pub fn cpu_wire_verdicts(frames: &[u8], offsets: &[u64], rng_seed: u64, committee: &CommitteeArrays) -> (Vec<i32>, Vec<u32>) {
    let n = offsets.len().saturating_sub(1);
    let na = committee.stakes.len();
    assert!(committee.keys.len() == 32 * na && committee.worker_offsets.len() == na + 1);
    let mut kinds = vec![0i32; n];
    let mut words = vec![0xffu32; n];
    let rc = unsafe {
        ffi::coa_cpu_wire_verdict_many(frames.as_ptr(), offsets.as_ptr(), n, rng_seed, committee.keys.as_ptr(),
                                       committee.stakes.as_ptr(), committee.worker_ids.as_ptr(),
                                       committee.worker_offsets.as_ptr(), na, kinds.as_mut_ptr(), words.as_mut_ptr(),
                                       CPU_THREADS)
    };
    cpu_status(rc, "PrimaryMessage frames (many)");
    (kinds, words)
}
