//go:build mi355x

// The MI355X build's server side of the verified reads: the marshalled
// schema.VerifiableTx of db.VerifiableTxByID (nil EntriesSpec) / VerifiableSet
// (pkg/database/database.go:1462-1528, :767-814) and schema.VerifiableEntry of
// db.VerifiableGet (:817-896) for many requests in one device pass
// (mh_verifiable_answer_pb_batch): ReadTx, ReadTxHeader, the tx readers of
// LinearProof / LinearAdvanceProof, the ahtree walks, tx.Proof and the
// protobuf marshalling, each distinct tx re-hashed once per call.  The store
// it reads -- tx log, commit log, ahtree -- is resident on the device; the
// index lookup and the value read stay with the Go database, which passes
// the marshalled schema.Entry.  TxAnswers (below) serves db.TxByID, db.TxScan
// and db.VerifiableTxByID under an EntriesSpec, the values read and checked
// on the device (mh_tx_answer_pb_batch).  Uncompiled in the build image (no Go
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
	"io"
	"time"
	"unsafe"

	"github.com/codenotary/immudb/embedded/internal/mi355x"
)

// the request kinds (enum MH_ANS_* of immustore_merkle.h)
const (
	ansTx    = 0
	ansEntry = 1
)

// ResidentStore names the device copies the answers are read from: the tx-log
// data after its appendable header (its allocation 256 bytes longer than
// TxLogLen), NTx commit-log entries and the ahtree over the Alh values.
type ResidentStore struct {
	Tree          *ReplicaTree
	TxLog         unsafe.Pointer
	TxLogLen      uint64
	CLog          unsafe.Pointer
	NTx           uint64
	CLogEntrySize int // 12 or 44 (cLogEntrySizeV1 / V2, immustore.go:122-123)
	MaxTxEntries  int
	MaxKeyLen     int
	// AnswerBytesHint is an upper bound of one batch's answer bytes, if the
	// caller knows one (it is raised to what a batch needed).  Zero sizes the
	// output by a first call that runs the whole device pass, the re-hash of
	// every distinct tx included, only to learn the length.
	AnswerBytesHint uint64
}

// AnswerRequest is one VerifiableTxByID / VerifiableGet request once the index
// has named the tx.
type AnswerRequest struct {
	Tx, ProveSinceTx uint64
	Key              []byte // VerifiableEntryAnswers: EncodeKey(vKey), as the tx stores it
	Entry            []byte // VerifiableEntryAnswers: the marshalled schema.Entry (may be empty)
}

func mapAnswerErr(st C.int) error {
	if st == C.MH_ERR_KEY_NOT_FOUND {
		return ErrKeyNotFound // Tx.IndexOf, tx.go:361-368
	}
	return mapErr(st)
}

// VerifiableTxAnswers returns the marshalled schema.VerifiableTx of every
// request (nil where errs[p] != nil).
func VerifiableTxAnswers(s *ResidentStore, reqs []AnswerRequest) (msgs [][]byte, errs []error, err error) {
	return verifiableAnswers(s, reqs, ansTx)
}

// VerifiableEntryAnswers returns the marshalled schema.VerifiableEntry of
// every request (nil where errs[p] != nil).
func VerifiableEntryAnswers(s *ResidentStore, reqs []AnswerRequest) (msgs [][]byte, errs []error, err error) {
	return verifiableAnswers(s, reqs, ansEntry)
}

func verifiableAnswers(s *ResidentStore, reqs []AnswerRequest, kind byte) ([][]byte, []error, error) {
	n := len(reqs)
	if s == nil || s.Tree == nil || s.Tree.h == nil {
		return nil, nil, ErrIllegalArguments
	}
	if n == 0 {
		return nil, nil, nil
	}
	// the request arrays live in C memory: the descriptor holds pointers
	nk, ne := 0, 0
	for _, r := range reqs {
		if kind == ansEntry {
			nk += len(r.Key)
			ne += len(r.Entry)
		}
	}
	alloc := func(bytes int) unsafe.Pointer { return C.calloc(1, C.size_t(bytes+8)) }
	kinds, txs, since := alloc(n), alloc(8*n), alloc(8*n)
	koff, eoff, keys, ents := alloc(8*(n+1)), alloc(8*(n+1)), alloc(nk), alloc(ne)
	for _, p := range []unsafe.Pointer{kinds, txs, since, koff, eoff, keys, ents} {
		defer C.free(p)
	}
	gk, gt, gs := unsafe.Slice((*byte)(kinds), n), unsafe.Slice((*uint64)(txs), n), unsafe.Slice((*uint64)(since), n)
	gko, geo := unsafe.Slice((*uint64)(koff), n+1), unsafe.Slice((*uint64)(eoff), n+1)
	gkb, geb := unsafe.Slice((*byte)(keys), nk+8), unsafe.Slice((*byte)(ents), ne+8)
	pk, pe := 0, 0
	for p, r := range reqs {
		gk[p], gt[p], gs[p] = kind, r.Tx, r.ProveSinceTx
		gko[p], geo[p] = uint64(pk), uint64(pe)
		if kind == ansEntry {
			pk += copy(gkb[pk:], r.Key)
			pe += copy(geb[pe:], r.Entry)
		}
	}
	gko[n], geo[n] = uint64(pk), uint64(pe)
	st := (*C.mh_answer_store)(C.calloc(1, C.size_t(unsafe.Sizeof(C.mh_answer_store{}))))
	defer C.free(unsafe.Pointer(st))
	st.txlog, st.txlog_len = (*C.uint8_t)(s.TxLog), C.uint64_t(s.TxLogLen)
	st.clog, st.ntx = (*C.uint8_t)(s.CLog), C.uint64_t(s.NTx)
	st.clog_entry_size = C.uint32_t(s.CLogEntrySize)
	st.max_entries, st.max_key_len = C.uint32_t(s.MaxTxEntries), C.uint32_t(s.MaxKeyLen)
	bt := (*C.mh_answer_batch)(C.calloc(1, C.size_t(unsafe.Sizeof(C.mh_answer_batch{}))))
	defer C.free(unsafe.Pointer(bt))
	bt.n = C.uint64_t(n)
	bt.kind, bt.tx, bt.prove_since = (*C.uint8_t)(kinds), (*C.uint64_t)(txs), (*C.uint64_t)(since)
	bt.keys, bt.key_off = (*C.uint8_t)(keys), (*C.uint64_t)(koff)
	bt.entries, bt.entry_off = (*C.uint8_t)(ents), (*C.uint64_t)(eoff)
	off := make([]C.uint64_t, n+1)
	status := make([]C.int32_t, n)
	// into the hinted capacity first; again, with the length the first call
	// reported, only when a message did not fit (off is complete either way)
	capBytes := s.AnswerBytesHint
	var out []byte
	for pass := 0; pass < 2; pass++ {
		out = make([]byte, capBytes+1)
		if rc := C.mh_verifiable_answer_pb_batch(s.Tree.h, st, bt, (*C.uint8_t)(unsafe.Pointer(&out[0])), C.uint64_t(capBytes), &off[0], &status[0]); rc != C.MH_OK {
			return nil, nil, mapAnswerErr(rc)
		}
		short := false
		for p := 0; p < n; p++ {
			short = short || status[p] == C.MH_ERR_BUFFER_TOO_SMALL
		}
		if !short {
			break
		}
		capBytes = uint64(off[n])
		s.AnswerBytesHint = capBytes
	}
	msgs, errs := make([][]byte, n), make([]error, n)
	for p := 0; p < n; p++ {
		if status[p] != C.MH_OK {
			errs[p] = mapAnswerErr(C.int(status[p]))
			continue
		}
		msgs[p] = out[off[p]:off[p+1]]
	}
	return msgs, errs, nil
}

// ---- db.TxByID / db.TxScan / db.VerifiableTxByID under an EntriesSpec

// the request kinds (enum MH_TXA_* of immustore_merkle.h)
const (
	TxAnswerTx         = 0 // schema.Tx: db.TxByID, one item of db.TxScan's TxList
	TxAnswerVerifiable = 1 // schema.VerifiableTx: db.VerifiableTxByID
)

// EntryTypeSpec and EntriesSpec mirror schema.EntryTypeSpec / schema.EntriesSpec
// (Action: schema.EntryTypeAction, EXCLUDE 0 .. RESOLVE 3); a nil pointer is a
// nil spec.
type EntryTypeSpec struct{ Action int32 }

type EntriesSpec struct {
	KvEntriesSpec, ZEntriesSpec, SqlEntriesSpec *EntryTypeSpec
}

// TxAnswerRequest is one TxByID / TxScan item / VerifiableTxByID request.
// ProveSinceTx is read for TxAnswerVerifiable only.  Spec nil: TxToProto.
type TxAnswerRequest struct {
	Kind             int
	Tx, ProveSinceTx uint64
	Spec             *EntriesSpec
}

func mapTxAnswerErr(st C.int) error {
	if st == C.MH_ERR_EOF {
		return io.EOF // readValueAt, immustore.go:3187; the vLog's ReadAt
	}
	return mapErr(st)
}

func specAction(s *EntryTypeSpec) byte {
	if s == nil {
		return C.MH_TXA_NO_SPEC
	}
	return byte(s.Action)
}

// TxAnswers returns the marshalled schema.Tx / schema.VerifiableTx of every
// request (nil where errs[p] != nil): db.serializeTx (database.go:1080-1231)
// and ImmuStore.ReadValue for many requests in one device pass.  tree may be
// nil when no request is TxAnswerVerifiable.  kv / z RESOLVE is not covered
// (ErrIllegalArguments for the whole call): such requests stay with the Go
// database.
func TxAnswers(store *ExportableStore, tree *ReplicaTree, reqs []TxAnswerRequest, now time.Time) (msgs [][]byte, errs []error, err error) {
	n := len(reqs)
	if store == nil || len(store.VLogs) > 127 {
		return nil, nil, ErrIllegalArguments
	}
	if n == 0 {
		return nil, nil, nil
	}
	ctx, err := mi355x.Context()
	if err != nil {
		return nil, nil, err
	}
	alloc := func(bytes int) unsafe.Pointer { return C.calloc(1, C.size_t(bytes+8)) }
	kinds, txs, since := alloc(n), alloc(8*n), alloc(8*n)
	has, kv, z, sql := alloc(n), alloc(n), alloc(n), alloc(n)
	for _, p := range []unsafe.Pointer{kinds, txs, since, has, kv, z, sql} {
		defer C.free(p)
	}
	gk, gt, gs := unsafe.Slice((*byte)(kinds), n), unsafe.Slice((*uint64)(txs), n), unsafe.Slice((*uint64)(since), n)
	gh, gkv, gz, gsql := unsafe.Slice((*byte)(has), n), unsafe.Slice((*byte)(kv), n), unsafe.Slice((*byte)(z), n), unsafe.Slice((*byte)(sql), n)
	for p, r := range reqs {
		gk[p], gt[p], gs[p] = byte(r.Kind), r.Tx, r.ProveSinceTx
		gkv[p], gz[p], gsql[p] = C.MH_TXA_NO_SPEC, C.MH_TXA_NO_SPEC, C.MH_TXA_NO_SPEC
		if r.Spec != nil {
			gh[p] = 1
			gkv[p], gz[p], gsql[p] = specAction(r.Spec.KvEntriesSpec), specAction(r.Spec.ZEntriesSpec), specAction(r.Spec.SqlEntriesSpec)
		}
	}
	st := (*C.mh_export_store)(C.calloc(1, C.size_t(unsafe.Sizeof(C.mh_export_store{}))))
	defer C.free(unsafe.Pointer(st))
	vl := (*C.mh_export_vlog)(C.calloc(C.size_t(len(store.VLogs)+1), C.size_t(unsafe.Sizeof(C.mh_export_vlog{}))))
	defer C.free(unsafe.Pointer(vl))
	gv := unsafe.Slice(vl, len(store.VLogs)+1)
	for k, v := range store.VLogs {
		gv[k].data = (*C.uint8_t)(v.Data)
		gv[k].first_off, gv[k].end_off = C.uint64_t(v.FirstOff), C.uint64_t(v.EndOff)
	}
	st.txlog, st.txlog_len = (*C.uint8_t)(store.TxLog), C.uint64_t(store.TxLogLen)
	st.clog, st.ntx = (*C.uint8_t)(store.CLog), C.uint64_t(store.NTx)
	st.clog_entry_size = C.uint32_t(store.CLogEntrySize)
	st.max_entries, st.max_key_len = C.uint32_t(store.MaxTxEntries), C.uint32_t(store.MaxKeyLen)
	st.vlogs, st.nvlogs = vl, C.uint32_t(len(store.VLogs))
	bt := (*C.mh_tx_answer_batch)(C.calloc(1, C.size_t(unsafe.Sizeof(C.mh_tx_answer_batch{}))))
	defer C.free(unsafe.Pointer(bt))
	bt.n = C.uint64_t(n)
	bt.kind, bt.tx, bt.prove_since = (*C.uint8_t)(kinds), (*C.uint64_t)(txs), (*C.uint64_t)(since)
	bt.has_spec, bt.kv_action = (*C.uint8_t)(has), (*C.uint8_t)(kv)
	bt.z_action, bt.sql_action = (*C.uint8_t)(z), (*C.uint8_t)(sql)
	bt.now_unix = C.int64_t(now.Unix())
	var th *C.mh_ahtree
	if tree != nil {
		th = tree.h
	}
	off := make([]C.uint64_t, n+1)
	status := make([]C.int32_t, n)
	// into the hinted capacity first; again, with the length the first call
	// reported, only when an answer did not fit (off is complete either way)
	capBytes := store.ExportBytesHint
	var out []byte
	for pass := 0; pass < 2; pass++ {
		out = make([]byte, capBytes+1)
		if rc := C.mh_tx_answer_pb_batch((*C.mh_ctx)(ctx), th, st, bt, (*C.uint8_t)(unsafe.Pointer(&out[0])), C.uint64_t(capBytes), &off[0], &status[0]); rc != C.MH_OK {
			return nil, nil, mapTxAnswerErr(rc)
		}
		short := false
		for p := 0; p < n; p++ {
			short = short || status[p] == C.MH_ERR_BUFFER_TOO_SMALL
		}
		if !short {
			break
		}
		capBytes = uint64(off[n])
		store.ExportBytesHint = capBytes
	}
	msgs, errs = make([][]byte, n), make([]error, n)
	for p := 0; p < n; p++ {
		if status[p] != C.MH_OK {
			// (an answer that fails on a value digest keeps a range of unspecified bytes: never sent)
			errs[p] = mapTxAnswerErr(C.int(status[p]))
			continue
		}
		msgs[p] = out[off[p]:off[p+1]]
	}
	return msgs, errs, nil
}

// TxScan frames the answers of consecutive TxAnswerTx requests (txs
// initialTx .. initialTx + limit - 1, every one under spec) as the marshalled
// schema.TxList of db.TxScan (database.go:1531-1583): every Tx as field 1
// (0x0a, varint length, body).  The first tx that fails ends the scan with its
// error, as Go's loop does.
func TxScan(store *ExportableStore, initialTx uint64, limit int, spec *EntriesSpec, now time.Time) ([]byte, error) {
	if limit < 0 {
		return nil, ErrIllegalArguments
	}
	reqs := make([]TxAnswerRequest, limit)
	for k := range reqs {
		reqs[k] = TxAnswerRequest{Kind: TxAnswerTx, Tx: initialTx + uint64(k), Spec: spec}
	}
	msgs, errs, err := TxAnswers(store, nil, reqs, now)
	if err != nil {
		return nil, err
	}
	var list []byte
	for k, m := range msgs {
		if errs[k] != nil {
			return nil, errs[k]
		}
		list = append(list, 0x0a)
		for v := uint64(len(m)); ; v >>= 7 {
			if v < 0x80 {
				list = append(list, byte(v))
				break
			}
			list = append(list, byte(v)|0x80)
		}
		list = append(list, m...)
	}
	return list, nil
}
