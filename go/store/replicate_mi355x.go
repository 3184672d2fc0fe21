//go:build mi355x

// The MI355X build's follower side of replication: ImmuStore.ReplicateTx
// (immustore.go:2772-2932) for a run of exported txs in one device pass
// (mh_replicate_tx_batch): the bytes of ExportTx parsed, hashed and checked
// against the exported headers on the device, the accepted prefix appended
// to the follower's ahtree.  The vLog and tx-log writes, indexing and the
// wait hubs stay with the Go store: hdrs and the entry records the call
// returns are what they need.  Uncompiled in the build image (no Go
// toolchain); see go/README.md.
package store

/*
#cgo CFLAGS: -I${SRCDIR}/../../third_party/immustore_amd/include
#cgo LDFLAGS: -L${SRCDIR}/../../third_party/immustore_amd -limmustore_merkle -Wl,-rpath,${SRCDIR}/../../third_party/immustore_amd
#include <stdlib.h>
#include "immustore_merkle.h"
*/
import "C"

import (
	"crypto/sha256"
	"fmt"
	"unsafe"

	"github.com/codenotary/immudb/embedded/internal/mi355x"
)

// ErrTxNotReached marks a tx behind the first refused one of its batch:
// ReplicateTx was never called for it.
var ErrTxNotReached = fmt.Errorf("%w: an earlier tx of the batch was refused", ErrIllegalState)

func mapReplErr(st C.int) error {
	switch st {
	case C.MH_ERR_NEWER_VERSION_OR_CORRUPTED:
		return ErrNewerVersionOrCorruptedData // immustore.go:91
	case C.MH_ERR_ILLEGAL_TRUNCATION_ARGUMENT:
		return ErrIllegalTruncationArgument // immustore.go:111
	case C.MH_ERR_NULL_KEY:
		return ErrNullKey // immustore.go:60
	case C.MH_ERR_MAX_KEY_LEN_EXCEEDED:
		return ErrMaxKeyLenExceeded // immustore.go:61
	case C.MH_ERR_MAX_VALUE_LEN_EXCEEDED:
		return ErrMaxValueLenExceeded // immustore.go:62
	case C.MH_ERR_MAX_TX_ENTRIES_EXCEEDED:
		return ErrMaxTxEntriesLimitExceeded // immustore.go:59
	case C.MH_ERR_TX_ALREADY_COMMITTED:
		return ErrTxAlreadyCommitted // immustore.go:58
	case C.MH_ERR_TX_OUT_OF_ORDER:
		return fmt.Errorf("%w: attempt to commit a tx in wrong order", ErrUnexpectedError) // :1716
	case C.MH_ERR_TX_NOT_REACHED:
		return ErrTxNotReached
	}
	return mapErr(st)
}

// ReplicaTree is the follower's ahtree with its dLog resident on the device
// (mh_ahtree): its size is the last precommitted tx id.
type ReplicaTree struct {
	h *C.mh_ahtree
}

func NewReplicaTree() (*ReplicaTree, error) {
	ctx, err := mi355x.Context()
	if err != nil {
		return nil, err
	}
	t := &ReplicaTree{}
	if st := C.mh_ahtree_new((*C.mh_ctx)(ctx), &t.h); st != C.MH_OK {
		return nil, mapErr(st)
	}
	return t, nil
}

func (t *ReplicaTree) Close() error {
	if t.h == nil {
		return nil
	}
	st := C.mh_ahtree_free(t.h)
	t.h = nil
	return mapErr(st)
}

func (t *ReplicaTree) Size() (uint64, error) {
	var n C.uint64_t
	if st := C.mh_ahtree_size(t.h, &n); st != C.MH_OK {
		return 0, mapErr(st)
	}
	return uint64(n), nil
}

// ReplicateOptions are the store's limits and the follower's chain state.
type ReplicateOptions struct {
	MaxTxEntries, MaxKeyLen, MaxValueLen int
	SkipIntegrityCheck                   bool              // ReplicateTx's skipIntegrityCheck
	DryRun                               bool              // verdicts only; the tree is left as it was
	PrevAlh                              [sha256.Size]byte // inmemPrecommittedAlh (immustore.go:464)
}

// ReplicateTxBatch applies exported txs in order, as ReplicateTx would one by
// one up to the precommit: accepted is the length of the prefix whose Alh
// values were appended to aht, hdrs their headers as precommitted (the built
// Eh), err the verdict of tx `accepted` when it is not the whole batch.
func ReplicateTxBatch(aht *ReplicaTree, exported [][]byte, opts ReplicateOptions) (accepted int, hdrs []*TxHeader, err error) {
	n := len(exported)
	if aht == nil || aht.h == nil {
		return 0, nil, ErrIllegalArguments
	}
	if n == 0 {
		return 0, nil, nil
	}
	total := 0
	for _, b := range exported {
		total += len(b)
	}
	var arena mi355x.Arena
	if err := arena.Ensure(total + 64); err != nil {
		return 0, nil, err
	}
	defer arena.Free()
	buf := arena.Bytes()
	off := make([]uint64, n+1)
	p := 0
	for k, b := range exported {
		off[k] = uint64(p)
		p += copy(buf[p:], b)
	}
	off[n] = uint64(p)
	// the batch descriptor lives in C memory: it holds pointers
	bt := (*C.mh_replicate_batch)(C.calloc(1, C.size_t(unsafe.Sizeof(C.mh_replicate_batch{}))))
	defer C.free(unsafe.Pointer(bt))
	coff := (*C.uint64_t)(C.malloc(C.size_t(8 * (n + 1))))
	defer C.free(unsafe.Pointer(coff))
	copy(unsafe.Slice((*uint64)(unsafe.Pointer(coff)), n+1), off)
	bt.n = C.uint64_t(n)
	bt.txs = (*C.uint8_t)(arena.Ptr())
	bt.tx_off = coff
	bt.max_entries = C.uint32_t(opts.MaxTxEntries)
	bt.max_key_len = C.uint32_t(opts.MaxKeyLen)
	bt.max_value_len = C.uint32_t(opts.MaxValueLen)
	if opts.SkipIntegrityCheck {
		bt.flags |= C.MH_REPL_SKIP_INTEGRITY
	}
	if opts.DryRun {
		bt.flags |= C.MH_REPL_DRY_RUN
	}
	for i := 0; i < sha256.Size; i++ {
		bt.prev_alh[i] = C.uint8_t(opts.PrevAlh[i])
	}
	status := make([]C.int32_t, n)
	ch := make([]C.mh_tx_header, n)
	md := make([]byte, n*C.MH_MAX_TX_METADATA_LEN)
	var acc C.uint64_t
	st := C.mh_replicate_tx_batch(aht.h, bt, &status[0], &acc, &ch[0], (*C.uint8_t)(unsafe.Pointer(&md[0])), nil, nil, nil, 0, nil)
	if st != C.MH_OK {
		return 0, nil, mapReplErr(st)
	}
	accepted = int(acc)
	hdrs = make([]*TxHeader, accepted)
	for k := 0; k < accepted; k++ {
		c := &ch[k]
		h := &TxHeader{ID: uint64(c.id), Ts: int64(c.ts), BlTxID: uint64(c.bl_tx_id),
			Version: int(c.version), NEntries: int(c.nentries)}
		copy(h.PrevAlh[:], C.GoBytes(unsafe.Pointer(&c.prev_alh[0]), sha256.Size))
		copy(h.Eh[:], C.GoBytes(unsafe.Pointer(&c.eh[0]), sha256.Size))
		copy(h.BlRoot[:], C.GoBytes(unsafe.Pointer(&c.bl_root[0]), sha256.Size))
		if c.md_len > 0 {
			h.Metadata = NewTxMetadata()
			if err := h.Metadata.ReadFrom(md[c.md_off : c.md_off+c.md_len]); err != nil {
				return k, hdrs[:k], err
			}
		}
		hdrs[k] = h
	}
	if accepted < n {
		err = mapReplErr(C.int(status[accepted]))
	}
	return accepted, hdrs, err
}
