//go:build mi355x

// The MI355X build's leader side of replication: ImmuStore.ExportTx
// (immustore.go:2621-2770) for a run of consecutive txs in one device pass
// (mh_export_tx_batch): readTx's re-hash of every record, readValueAt's
// SHA-256 of every value against its stored hVal, and the bytes ReplicateTx
// takes, from a store whose tx log, commit log and value logs are resident on
// the device.  The blobs are what ReplicateTxs (replicate_mi355x.go) reads on
// the follower.  Uncompiled in the build image (no Go toolchain); see
// go/README.md.
package store

/*
#cgo CFLAGS: -I${SRCDIR}/../../third_party/immustore_amd/include
#cgo LDFLAGS: -L${SRCDIR}/../../third_party/immustore_amd -limmustore_merkle -Wl,-rpath,${SRCDIR}/../../third_party/immustore_amd
#include <stdlib.h>
#include "immustore_merkle.h"
*/
import "C"

import (
	"unsafe"

	"github.com/codenotary/immudb/embedded/internal/mi355x"
)

// ResidentVLog is one value log, or the part of it that is on the device:
// Data[0] is the log's byte FirstOff, bytes [FirstOff, EndOff) are resident,
// and the allocation is 256 bytes longer.
type ResidentVLog struct {
	Data             unsafe.Pointer
	FirstOff, EndOff uint64
}

// ExportableStore names the device copies ExportTxs reads: the tx-log data
// after its appendable header (its allocation 256 bytes longer than
// TxLogLen), NTx commit-log entries -- committed or precommitted, as
// allowPrecommitted decides -- and the value logs, VLogs[k] being vLog id k+1.
type ExportableStore struct {
	TxLog         unsafe.Pointer
	TxLogLen      uint64
	CLog          unsafe.Pointer
	NTx           uint64
	CLogEntrySize int // 12 or 44 (cLogEntrySizeV1 / V2, immustore.go:122-123)
	MaxTxEntries  int
	MaxKeyLen     int
	VLogs         []ResidentVLog
	// ExportBytesHint is an upper bound of one run's exported bytes, if the
	// caller knows one (it is raised to what a run needed).  Zero sizes the
	// output by a first call that runs the whole device pass only to learn the
	// length.
	ExportBytesHint uint64
}

// ExportTxs returns ExportTx(firstTx + k, allowPrecommitted, false, tx) for k
// in [0, count): blobs[k] is nil where errs[k] != nil; truncated[k] tells
// whether blob k carries value hashes instead of values.
func ExportTxs(s *ExportableStore, firstTx uint64, count int) (blobs [][]byte, truncated []bool, errs []error, err error) {
	if s == nil || count < 0 || len(s.VLogs) > 127 {
		return nil, nil, nil, ErrIllegalArguments
	}
	if count == 0 {
		return nil, nil, nil, nil
	}
	ctx, err := mi355x.Context()
	if err != nil {
		return nil, nil, nil, err
	}
	// the descriptor and its vLog table live in C memory: they hold pointers
	st := (*C.mh_export_store)(C.calloc(1, C.size_t(unsafe.Sizeof(C.mh_export_store{}))))
	defer C.free(unsafe.Pointer(st))
	vl := (*C.mh_export_vlog)(C.calloc(C.size_t(len(s.VLogs)+1), C.size_t(unsafe.Sizeof(C.mh_export_vlog{}))))
	defer C.free(unsafe.Pointer(vl))
	gv := unsafe.Slice(vl, len(s.VLogs)+1)
	for k, v := range s.VLogs {
		gv[k].data = (*C.uint8_t)(v.Data)
		gv[k].first_off, gv[k].end_off = C.uint64_t(v.FirstOff), C.uint64_t(v.EndOff)
	}
	st.txlog, st.txlog_len = (*C.uint8_t)(s.TxLog), C.uint64_t(s.TxLogLen)
	st.clog, st.ntx = (*C.uint8_t)(s.CLog), C.uint64_t(s.NTx)
	st.clog_entry_size = C.uint32_t(s.CLogEntrySize)
	st.max_entries, st.max_key_len = C.uint32_t(s.MaxTxEntries), C.uint32_t(s.MaxKeyLen)
	st.vlogs, st.nvlogs = vl, C.uint32_t(len(s.VLogs))
	off := make([]C.uint64_t, count+1)
	status := make([]C.int32_t, count)
	trunc := make([]C.uint8_t, count)
	// into the hinted capacity first; again, with the length the first call
	// reported, only when a blob did not fit (off is complete either way)
	capBytes := s.ExportBytesHint
	var out []byte
	for pass := 0; pass < 2; pass++ {
		out = make([]byte, capBytes+1)
		if rc := C.mh_export_tx_batch((*C.mh_ctx)(ctx), st, C.uint64_t(firstTx), C.uint64_t(count), (*C.uint8_t)(unsafe.Pointer(&out[0])), C.uint64_t(capBytes), &off[0], &status[0], &trunc[0]); rc != C.MH_OK {
			return nil, nil, nil, mapErr(rc)
		}
		short := false
		for k := 0; k < count; k++ {
			short = short || status[k] == C.MH_ERR_BUFFER_TOO_SMALL
		}
		if !short {
			break
		}
		capBytes = uint64(off[count])
		s.ExportBytesHint = capBytes
	}
	blobs, truncated, errs = make([][]byte, count), make([]bool, count), make([]error, count)
	for k := 0; k < count; k++ {
		if status[k] != C.MH_OK {
			// (a tx that fails on a value digest keeps a range of unspecified bytes: never sent)
			errs[k] = mapErr(C.int(status[k]))
			continue
		}
		blobs[k] = out[off[k]:off[k+1]]
		truncated[k] = trunc[k] != 0
	}
	return blobs, truncated, errs, nil
}
