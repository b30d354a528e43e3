//! Whole headers and votes through the engine's aggregation queue:
//! `VerifyService::header(..)` and `VerifyService::vote(..)` over
//! `coa_queue_submit_header` / `coa_queue_submit_vote` (include/coa_verify.h).
//!
//! `VerifyService::verify` (service.rs) takes a bare (digest, key, signature)
//! triple: the producer hashes `Vote::digest` itself, the header's id check
//! (primary/src/messages.rs:49-51) stays with `Core`, and a large window
//! treats every signer as a stranger.  These two requests hand the engine the
//! whole message instead, so the window runs on the registered committee's
//! key combs with `Header::digest` checked and `Vote::digest` hashed on the
//! device, and an author outside the committee is still decided exactly (the
//! queue's resolver).
//!
//! The requests go to a queue of their own, made on first use with the
//! service's settings (COA_SERVICE_MAX_BATCH / COA_SERVICE_MAX_DELAY_US,
//! idle launch as `VerifyService::new`): a window of headers and votes alone
//! takes the publish route of the message latency kernel (no copy back, no
//! event wait), which a window shared with certificates would not.  Each
//! request is submitted by the calling task -- the queue copies it under a
//! per-thread shard lock and never blocks on the device -- and answered
//! through a `oneshot`, as the service's other requests are.
//!
//! Wiring (crypto/src/lib.rs): `pub mod message_service;`.
use crate::coa_ffi as ffi;
use crate::degrade;
use crate::service::VerifyService;
use crate::{CryptoError, Digest, PublicKey};
use std::os::raw::{c_int, c_void};
use tokio::sync::oneshot;

/// The engine's status byte, or its failure status.
type Reply = Result<u8, c_int>;

struct Queue(*mut ffi::CoaQueue);
unsafe impl Send for Queue {}
unsafe impl Sync for Queue {}

/// The process's message queue (`std::sync::Once`: the reference pins Rust
/// 1.51.0).  Never destroyed: it lives as long as the node.
fn message_queue() -> *mut ffi::CoaQueue {
    static INIT: std::sync::Once = std::sync::Once::new();
    static mut QUEUE: *const Queue = std::ptr::null();
    unsafe {
        INIT.call_once(|| {
            let batch = std::env::var("COA_SERVICE_MAX_BATCH").ok().and_then(|v| v.parse().ok()).unwrap_or(65_536);
            let delay = std::env::var("COA_SERVICE_MAX_DELAY_US").ok().and_then(|v| v.parse().ok()).unwrap_or(500);
            let queue = ffi::coa_queue_create(batch, delay);
            assert!(!queue.is_null(), "MI355X verification engine: coa_queue_create failed: {}", ffi::last_error());
            let idle: u32 =
                std::env::var("COA_SERVICE_IDLE_LAUNCH").ok().and_then(|v| v.parse().ok()).unwrap_or(1u32).min(64);
            let rc = ffi::coa_queue_set_idle_launch(queue, idle);
            assert_eq!(rc, ffi::COA_OK, "MI355X verification engine: coa_queue_set_idle_launch({}) failed", idle);
            QUEUE = Box::into_raw(Box::new(Queue(queue)));
        });
        (*QUEUE).0
    }
}

/// coa_verdict_cb of both kinds: one status byte, once per queued request, on
/// the engine's completion or resolver thread.  Never panics.
unsafe extern "C" fn on_message(user: *mut c_void, status: c_int, verdicts: *const u8, n: usize) {
    let sender = Box::from_raw(user as *mut oneshot::Sender<Reply>);
    let reply = if status != ffi::COA_OK {
        Err(status)
    } else if verdicts.is_null() || n != 1 {
        Err(ffi::COA_EINVAL)
    } else {
        Ok(*verdicts)
    };
    let _ = sender.send(reply);
}

impl VerifyService {
    /// The crypto of `Header::verify` (primary/src/messages.rs:49-51, 64-66):
    /// the COA_CERT_BAD_HEADER_ID | COA_CERT_BAD_HEADER_SIG bits (0 = both
    /// Ok).  `header_input` is what `Header::digest` hashes (:70-84).
    pub async fn header(&self, header_input: &[u8], id: &Digest, author: &PublicKey, signature: [u8; 64]) -> u8 {
        let (sender, receiver) = oneshot::channel();
        // (the raw pointer stays inside this block: the future remains Send)
        let rc = {
            let user = Box::into_raw(Box::new(sender)) as *mut c_void;
            let rc = unsafe {
                ffi::coa_queue_submit_header(message_queue(), header_input.as_ptr(), header_input.len(),
                                             id.0.as_ptr(), author.0.as_ptr(), signature.as_ptr(), Some(on_message),
                                             user)
            };
            if rc != ffi::COA_OK {
                // not queued: the callback will never run
                let _unqueued = unsafe { Box::from_raw(user as *mut oneshot::Sender<Reply>) };
            }
            rc
        };
        let reply = if rc != ffi::COA_OK {
            Err(rc)
        } else {
            receiver.await.expect("Failed to receive status from the message queue")
        };
        match reply {
            Ok(bits) => bits,
            Err(status) => {
                degrade::engine_failed(status, "every context failed", "VerifyService::header");
                degrade::cpu_header_bits(header_input, &[0, header_input.len() as u64], &id.0, &author.0, &signature)[0]
            }
        }
    }

    /// `Vote::verify`'s signature check (primary/src/messages.rs:139-141) over
    /// `Vote::digest` (:145-153), which the engine hashes from `id`, `round`
    /// and `origin`.
    pub async fn vote(&self, id: &Digest, round: u64, origin: &PublicKey, author: &PublicKey,
                      signature: [u8; 64]) -> Result<(), CryptoError> {
        let (sender, receiver) = oneshot::channel();
        let rc = {
            let user = Box::into_raw(Box::new(sender)) as *mut c_void;
            let rc = unsafe {
                ffi::coa_queue_submit_vote(message_queue(), id.0.as_ptr(), round, origin.0.as_ptr(),
                                           author.0.as_ptr(), signature.as_ptr(), Some(on_message), user)
            };
            if rc != ffi::COA_OK {
                let _unqueued = unsafe { Box::from_raw(user as *mut oneshot::Sender<Reply>) };
            }
            rc
        };
        let reply = if rc != ffi::COA_OK {
            Err(rc)
        } else {
            receiver.await.expect("Failed to receive verdict from the message queue")
        };
        let byte = match reply {
            Ok(byte) => byte,
            Err(status) => {
                degrade::engine_failed(status, "every context failed", "VerifyService::vote");
                degrade::cpu_vote_verdicts(&id.0, &[round], &origin.0, &author.0, &signature)[0]
            }
        };
        if byte == 0 {
            Ok(())
        } else {
            Err(CryptoError::new())
        }
    }
}
